"""The float64 statement of an `ops.gemm` launch (tests/helpers/gemm_ref.py) pinned WITHOUT any kernel: every feature it
models is compared with torch's own float64 operators (F.conv2d and autograd through it, F.gelu / F.silu and their autograd)
at float64 agreement, <= 1e-12 relative.  The launches are real `functools.partial(ops.gemm, ...)` objects over CPU float64
tensors — they are only read, never called — with the packed weights the engines use (packing.conv3x3_fwd / conv3x3_dgrad /
_chunk_major / geglu_interleave)."""
import math
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from helpers import gemm_ref as G
from helpers.checks import ops as _ops

TOL = 1e-12


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def close(name, got, ref):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    err = ((got - ref).norm() / ref.norm()).item()
    worst = ((got - ref).abs().max() / ref.abs().max()).item()
    assert err <= TOL and worst <= TOL, f"{name}: rel {err:.2e}, max {worst:.2e}"


def _nhwc_wide(x, ldx):
    """[B, C, H, W] -> the NHWC image inside a wider buffer (pixel stride ldx > C: a column slice of a concat buffer); the
    neighbouring columns hold large values a wrong stride would pick up"""
    Bn, Cc, H, W = x.shape
    buf = torch.full((Bn * H * W, ldx), 1e6, dtype=torch.float64)
    off = (ldx - Cc) // 2
    view = buf[:, off:off + Cc]
    view.copy_(x.permute(0, 2, 3, 1).reshape(-1, Cc))
    return view


CONV_CASES = ["s1", "s2p1", "s2vae", "ups"]


def _conv_case(case, x, w):
    """F.conv2d form of the case and the conv dict of its forward gather"""
    Bn, Ci, H, W = x.shape
    if case == "s1":
        fwd = lambda t: F.conv2d(t, w, None, padding=1)
        d = dict(Hi=H, Wi=W, Ho=H, Wo=W, stride=1, pad_t=1, pad_l=1, ups=0)
    elif case == "s2p1":
        fwd = lambda t: F.conv2d(t, w, None, stride=2, padding=1)
        d = dict(Hi=H, Wi=W, Ho=H // 2, Wo=W // 2, stride=2, pad_t=1, pad_l=1, ups=0)
    elif case == "s2vae":  # AutoencoderKL's Downsample2D: pad (0, 1, 0, 1), then padding 0
        fwd = lambda t: F.conv2d(F.pad(t, (0, 1, 0, 1)), w, None, stride=2, padding=0)
        d = dict(Hi=H, Wi=W, Ho=H // 2, Wo=W // 2, stride=2, pad_t=0, pad_l=0, ups=0)
    else:
        fwd = lambda t: F.conv2d(F.interpolate(t, scale_factor=2.0, mode="nearest"), w, None, padding=1)
        d = dict(Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, stride=1, pad_t=1, pad_l=1, ups=1)
    return fwd, d


@pytest.mark.parametrize("korder", [0, 1], ids=["tap-major", "chunk-major"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_forward_gather_is_conv2d(case, korder):
    from view_neti_amd import packing
    Bn, Ci, Co, H, W = 2, 128, 24, 6, 10  # two 64-channel chunks (the K orders differ), H != W, even (stride 2)
    x, w, bias = rnd(Bn, Ci, H, W, seed=1), rnd(Co, Ci, 3, 3, seed=2, scale=0.05), rnd(Co, seed=3)
    fwd, d = _conv_case(case, x, w)
    ref = fwd(x) + bias.view(1, Co, 1, 1)
    Ho, Wo = ref.shape[2], ref.shape[3]
    assert (Ho, Wo) == (d["Ho"], d["Wo"])
    ldx = Ci + 16
    conv = dict(d, mode=1, Ci=Ci, ldx=ldx, korder=korder)
    M = Bn * Ho * Wo
    out = torch.zeros(M, Co + 8, dtype=torch.float64)[:, :Co]
    f = partial(_ops().gemm, _nhwc_wide(x, ldx), packing.conv3x3_fwd(w, cm=bool(korder)), out, bias=bias, conv=conv, M=M)
    got = G.reference(f)
    assert got.out2 is None and got.gn is None
    close(f"conv {case}", got.out.view(Bn, Ho, Wo, Co), ref.permute(0, 2, 3, 1))
    g = G.geometry(f)
    assert (g.M, g.N, g.K, g.batch) == (M, Co, 9 * Ci, 1) and g.out_shape == (1, M, Co) and g.out_strides[1] == Co + 8


@pytest.mark.parametrize("korder", [0, 1], ids=["tap-major", "chunk-major"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_transposed_gather_is_the_input_gradient(case, korder):
    """mode 2 with packing.conv3x3_dgrad weights against autograd's input gradient of F.conv2d; the fused-upsample conv has
    a stride-1 transposed gather on the upsampled grid, whose 2 x 2 sums are the gradient of the low-resolution input"""
    from view_neti_amd import packing
    Bn, Ci, Co, H, W = 2, 8, 128, 6, 10  # dy has Co channels (the gather's Ci, two chunks), dx has Ci
    x = rnd(Bn, Ci, H, W, seed=4).requires_grad_(True)
    w = rnd(Co, Ci, 3, 3, seed=5, scale=0.05)
    fwd, d = _conv_case(case, x, w)
    y = fwd(x)
    dy = rnd(*y.shape, seed=6)
    y.backward(dy)
    Hy, Wy = y.shape[2], y.shape[3]
    Hx, Wx = (2 * H, 2 * W) if case == "ups" else (H, W)  # the grid the gather produces
    ldx = Co + 8
    conv = dict(mode=2, Hi=Hy, Wi=Wy, Ci=Co, Ho=Hx, Wo=Wx, stride=d["stride"], pad_t=d["pad_t"], pad_l=d["pad_l"], ups=0,
                ldx=ldx, korder=korder)
    wd = packing.conv3x3_dgrad(w)
    if korder:
        wd = packing._chunk_major(wd, Ci, Co)
    M = Bn * Hx * Wx
    f = partial(_ops().gemm, _nhwc_wide(dy, ldx), wd, torch.zeros(M, Ci, dtype=torch.float64), conv=conv, M=M)
    got = G.reference(f).out.view(Bn, Hx, Wx, Ci)
    if case == "ups":
        got = got.view(Bn, H, 2, W, 2, Ci).sum((2, 4))
    close(f"dgrad {case}", got, x.grad.permute(0, 2, 3, 1))


def test_geglu_forward_and_backward():
    from view_neti_amd import packing
    M, C, F4 = 10, 64, 48
    x, W, b = rnd(M, C, seed=7), rnd(2 * F4, C, seed=8, scale=0.2), rnd(2 * F4, seed=9)
    p_out = torch.zeros(M, 2 * F4, dtype=torch.float64)
    gg_out = torch.zeros(M, F4 + 8, dtype=torch.float64)[:, :F4]
    f = partial(_ops().gemm, x, packing.geglu_interleave(W), p_out, bias=packing.geglu_interleave(b), out2=gg_out, geglu=1,
                split_k=1)
    got = G.reference(f)
    pre = (x @ W.t() + b).detach().requires_grad_(True)   # [h | g], the reference's own order
    idx = packing.geglu_interleave_index(2 * F4)
    act = pre[:, :F4] * F.gelu(pre[:, F4:])
    close("geglu 1 pre-activation (interleaved)", got.out, pre.detach()[:, idx])
    close("geglu 1 h * gelu(g)", got.out2, act.detach())
    assert G.geometry(f).out2_shape == (M, F4) and G.geometry(f).out2_strides == (F4 + 8, 1)
    # backward: d = dy @ W2 is the [M][F4] GEMM result; the launch writes [M][2 * F4] against the saved pre-activation
    dy, W2 = rnd(M, C, seed=10), rnd(C, F4, seed=11, scale=0.2)
    d = dy @ W2
    (act * d).sum().backward()
    gate = torch.full((M, 2 * F4 + 8), 1e6, dtype=torch.float64)[:, :2 * F4]
    gate.copy_(got.out)
    f2 = partial(_ops().gemm, dy, W2.t().contiguous(), torch.zeros(M, 2 * F4, dtype=torch.float64), gate=gate,
                 gate_act=3, geglu=2, split_k=1)
    close("geglu 2", G.reference(f2).out, pre.grad[:, idx])
    g2 = G.geometry(f2)
    assert (g2.N, g2.out_shape) == (F4, (1, M, 2 * F4))


@pytest.mark.parametrize("kind", [1, 2, 3], ids=["silu", "quick_gelu", "gelu"])
def test_gate_and_activations_are_autograd(kind):
    fn = {1: F.silu, 2: lambda t: t * torch.sigmoid(1.702 * t), 3: F.gelu}[kind]
    M, N, K = 9, 20, 64
    A, B, bias = rnd(M, K, seed=12), rnd(N, K, seed=13, scale=0.2), rnd(N, seed=14)
    pre = (rnd(M, N + 4, seed=15) * 2.0)[:, 2:2 + N]
    xg = pre.clone().requires_grad_(True)
    fn(xg).sum().backward()
    f = partial(_ops().gemm, A, B, torch.zeros(M, N, dtype=torch.float64), bias=bias, gate=pre, gate_act=kind,
                out2=torch.zeros(M, N, dtype=torch.float64), act2=kind)
    got = G.reference(f)
    want = (A @ B.t() + bias) * xg.grad
    close(f"gate act {kind}", got.out, want)
    close(f"out2 act {kind}", got.out2, fn(want))
    f = partial(_ops().gemm, A, B, torch.zeros(M, N, dtype=torch.float64), bias=bias, act=kind, alpha=0.25)
    close(f"act {kind} with alpha", G.reference(f).out, fn(0.25 * (A @ B.t()) + bias))


def test_rowadd_resid_in_place_and_overrides():
    """the row-add group of a row, a residual that IS the output (read before it is replaced), M / N / K / lda / ldc
    overrides on wider buffers, and the GroupNorm sums of the result"""
    M, N, K, rpg, G_ = 24, 16, 64, 6, 4
    Abig, Bbig = rnd(M + 3, K + 64, seed=16), rnd(N + 5, K + 64, seed=17, scale=0.2)
    radd = rnd(M // rpg, N + 8, seed=18)[:, :N]
    outbig = rnd(M, N + 8, seed=19)
    out = outbig[:, 4:4 + N]
    before = out.clone()
    sums = torch.zeros(M // 12, 8, G_, 4, dtype=torch.int64)
    f = partial(_ops().gemm, Abig, Bbig, out, rowadd=radd, rows_per_group=rpg, resid=out, M=M, N=N, K=K,
                gn_sums=sums, gn_hw=12, gn_groups=G_, gn_slots=8)
    got = G.reference(f)
    want = Abig[:M, :K] @ Bbig[:N, :K].t() + radd.repeat_interleave(rpg, 0) + before
    close("rowadd + in-place resid", got.out, want)
    assert torch.equal(out, before), "the reference only reads"
    v = want.view(M // 12, 12, G_, N // G_)
    close("gn sum", got.gn[..., 0], v.sum((1, 3)))
    close("gn sumsq", got.gn[..., 1], (v * v).sum((1, 3)))
    g = G.geometry(f)
    assert (g.M, g.N, g.K) == (M, N, K) and g.out_strides == (0, N + 8, 1)
    # lda / ldc given explicitly (the batched attention GEMMs pass them)
    f = partial(_ops().gemm, Abig[:, 8:], Bbig, outbig, M=M, N=N, K=K, lda=K + 64, ldc=N + 8)
    close("lda override", G.reference(f).out, Abig[:M, 8:8 + K] @ Bbig[:N, :K].t())


def test_batch_strides():
    """the three batch strides: stacked weights (the UNet's K / V projections), a shared B (stride 0), operands that are
    column slices of one buffer with the batch stride reaching past the view (the VAE's q . k^T)"""
    n, M, N, K = 3, 7, 12, 64
    A, B = rnd(n, M, K, seed=20), rnd(n, N, K, seed=21, scale=0.2)
    out = torch.zeros(n, M, N, dtype=torch.float64)
    f = partial(_ops().gemm, A[0], B[0], out[0], batch=n, strideA=M * K, strideB=N * K, strideC=M * N)
    got = G.reference(f)
    close("batched, stacked", got.out, A @ B.transpose(1, 2))
    assert G.geometry(f).out_shape == (n, M, N) and G.geometry(f).out_strides == (M * N, N, 1)
    f = partial(_ops().gemm, A[0], B[1], out[0], batch=n, strideA=M * K, strideB=0, strideC=M * N)
    close("batched, shared B", G.reference(f).out, A @ B[1].t())
    # q | k | v column slices of one [n * M][3 * K] buffer; scores into rows of ld 16 > M; resid batched like the output
    qkv = rnd(n * M, 3 * K, seed=22)
    q, k = qkv[:, :K], qkv[:, K:2 * K]
    res = rnd(n, M, 16, seed=23)
    f = partial(_ops().gemm, q, k, torch.zeros(n, M, 16, dtype=torch.float64), alpha=K ** -0.5, batch=n,
                strideA=M * 3 * K, strideB=M * 3 * K, strideC=M * 16, M=M, N=M, K=K, lda=3 * K, ldc=16, resid=res[0, :, :M])
    want = K ** -0.5 * (q.reshape(n, M, K) @ k.reshape(n, M, K).transpose(1, 2)) + res[:, :, :M]
    close("batched, column slices", G.reference(f).out, want)


def test_geglu_column_order_round_trip():
    from view_neti_amd import packing
    x = rnd(5, 32, seed=24)
    h, g = G.geglu_split(x)
    assert torch.equal(G.geglu_join(h, g), x)
    idx = packing.geglu_interleave_index(32)
    assert torch.equal(torch.cat((h, g), 1)[:, idx], x)
    assert math.isclose(float(G.act(torch.tensor([0.7], dtype=torch.float64), 3)), float(F.gelu(torch.tensor([0.7], dtype=torch.float64))),
                        rel_tol=1e-14)
