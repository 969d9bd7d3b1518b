"""A float64 statement of ONE `ops.gemm` launch, read off the bound launch itself.

`reference(f)` takes a `functools.partial` over `ops.gemm` (the form the engines' schedules hold) and reads nothing but
its `args` and `keywords`; plain torch float64, nothing of the library is imported or called.  It states what
include/vneti.h documents for vneti_gemm_desc:

    acc[b][m][n] = sum_k A[b][m][k] * B[b][n][k]          A, B: strided matrices (lda / ldb, batch strides), or, with
                                                          `conv`, A = the explicit im2col matrix of an NHWC image
    x   = act(alpha * acc + bias[n])
    x  += rowadd[m // rows_per_group][n]
    x  += resid[b][m][n]                                  (resid may be the output's previous content: read first)
    x  *= act'(gate[m][n])                                (gate_act)
    out = x ;  out2 = act2(x)
    geglu 1: out = x in the interleaved column order [h0..h3 g0..g3 h4..h7 g4..g7 ...]; out2[m][4q+e] = h * gelu(g)
    geglu 2: x is d[M][N]; gate = the saved interleaved pre-activation [M][2N]; out[M][2N] = (d * gelu(g), d * h * gelu'(g))
             in the same interleaved order
    gn_sums: (sum x, sum x^2) over the gn_hw rows of an image and the N / gn_groups columns of a group

The ORDER of the epilogue's intermediate 16-bit roundings is not modelled (test_gemm_epilogue_adds_round_like_f32 pins it);
everything here is exact float64 arithmetic on the launch's operands as they are in memory.

`geometry(f)` gives the launch's logical extents (what the kernel may write), for the tests that check the surroundings.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

Ref = namedtuple("Ref", "out out2 gn")  # out: [M, Nw] ([batch, M, Nw] when batched); out2: [M, N2] or None; gn: [img, G, 2] or None
Geometry = namedtuple("Geometry", "M N K batch out_shape out_strides out2_shape out2_strides")


def _strided(t, shape, strides):
    """the elements the kernel addresses from t's pointer with these element strides (may reach past t's own shape, as the
    batched launches do through their batch stride)"""
    return torch.as_strided(t, shape, strides, t.storage_offset())


def _ld(t):
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


def geometry(f) -> Geometry:
    kw = f.keywords
    A, B, out = f.args[:3]
    conv = kw.get("conv")
    N = kw.get("N") if kw.get("N") is not None else B.shape[-2]
    K = kw.get("K") if kw.get("K") is not None else B.shape[-1]
    M = kw.get("M") if (conv is not None or kw.get("M") is not None) else A.shape[-2]
    batch = kw.get("batch") or 1
    geglu = kw.get("geglu") or 0
    ldc = kw.get("ldc") if kw.get("ldc") is not None else _ld(out)
    Nw = 2 * N if geglu == 2 else N
    out2 = kw.get("out2")
    o2s = o2st = None
    if out2 is not None:
        o2s, o2st = (M, N // 2 if geglu == 1 else N), (_ld(out2), 1)
    return Geometry(M, N, K, batch, (batch, M, Nw), (kw.get("strideC") or 0, ldc, 1), o2s, o2st)


# ---------------------------------------------------------------------------------------------- activations, float64
def _phi(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act(x, kind):
    """0 none, 1 SiLU, 2 quick-GELU, 3 exact GELU"""
    if kind == 0:
        return x
    if kind == 1:
        return x * torch.sigmoid(x)
    if kind == 2:
        return x * torch.sigmoid(1.702 * x)
    if kind == 3:
        return x * _phi(x)
    raise ValueError(f"act {kind}")


def act_grad(x, kind):
    if kind == 1:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if kind == 2:
        s = torch.sigmoid(1.702 * x)
        return s + 1.702 * x * s * (1.0 - s)
    if kind == 3:
        return _phi(x) + x * _pdf(x)
    raise ValueError(f"gate_act {kind}")


# ---------------------------------------------------------------------------------------------- implicit convolution
def im2col(A, conv, M) -> torch.Tensor:
    """the explicit [M][9 * Ci] float64 matrix the implicit convolution multiplies: row m = (image, oy, ox), column
    tap * Ci + ci with tap = dy * 3 + dx (korder 0), or (ci // 64, tap, ci % 64) (korder 1).
    mode 1: in(oy * stride + dy - pad_t, ox * stride + dx - pad_l) of the image, nearest-2x upsampled first when `ups`
            (Hi, Wi are then the low-resolution dims); mode 2: in((oy + pad_t - dy) / stride, (ox + pad_l - dx) / stride)
            where both divisions are exact; zero outside the image."""
    Hi, Wi, Ci, Ho, Wo = (int(conv[k]) for k in ("Hi", "Wi", "Ci", "Ho", "Wo"))
    stride, pad_t, pad_l = int(conv["stride"]), int(conv["pad_t"]), int(conv["pad_l"])
    ldx, mode = int(conv["ldx"]), int(conv["mode"])
    assert M % (Ho * Wo) == 0
    Bn = M // (Ho * Wo)
    img = _strided(A, (Bn, Hi, Wi, Ci), (Hi * Wi * ldx, Wi * ldx, ldx, 1)).double()
    if conv.get("ups"):
        assert mode == 1 and stride == 1
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
    Hs, Ws = img.shape[1], img.shape[2]
    dev = img.device
    oy = torch.arange(Ho, device=dev).view(Ho, 1)
    ox = torch.arange(Wo, device=dev).view(1, Wo)
    col = torch.zeros(Bn, Ho, Wo, 9, Ci, dtype=torch.float64, device=dev)
    for dy in range(3):
        for dx in range(3):
            if mode == 1:
                iy, ix = oy * stride + dy - pad_t, ox * stride + dx - pad_l
                ok = (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws)
            elif mode == 2:
                ny, nx = oy + pad_t - dy, ox + pad_l - dx
                ok = (ny >= 0) & (nx >= 0) & (ny % stride == 0) & (nx % stride == 0)
                iy, ix = torch.div(ny, stride, rounding_mode="floor"), torch.div(nx, stride, rounding_mode="floor")
                ok = ok & (iy < Hs) & (ix < Ws)
            else:
                raise ValueError(f"conv mode {mode}")
            iy, ix = iy.clamp(0, Hs - 1).expand(Ho, Wo), ix.clamp(0, Ws - 1).expand(Ho, Wo)
            col[:, :, :, dy * 3 + dx, :] = img[:, iy, ix, :] * ok.expand(Ho, Wo).view(1, Ho, Wo, 1).double()
    if conv.get("korder"):
        assert Ci % 64 == 0
        col = col.view(Bn, Ho, Wo, 9, Ci // 64, 64).permute(0, 1, 2, 4, 3, 5)
    return col.reshape(M, 9 * Ci)


# ---------------------------------------------------------------------------------------------- GEGLU column order
def geglu_split(x):
    """[M][N] in the interleaved order (position 8q + e: h[4q + e] for e < 4, g[4q + e - 4] for e >= 4) -> h, g [M][N / 2]"""
    M, N = x.shape
    assert N % 8 == 0
    v = x.reshape(M, N // 8, 2, 4)
    return v[:, :, 0, :].reshape(M, N // 2), v[:, :, 1, :].reshape(M, N // 2)


def geglu_join(h, g):
    M, F = h.shape
    return torch.stack((h.reshape(M, F // 4, 4), g.reshape(M, F // 4, 4)), 2).reshape(M, 2 * F)


def gn_sums(x, hw, groups):
    """[M][N] -> [M / hw][groups][2]: (sum, sum of squares) per (image of hw rows, group of N / groups columns)"""
    M, N = x.shape
    v = x.double().reshape(M // hw, hw, groups, N // groups)
    return torch.stack((v.sum((1, 3)), (v * v).sum((1, 3))), -1)


# ---------------------------------------------------------------------------------------------- the launch
def reference(f) -> Ref:
    kw = f.keywords
    A, B = f.args[:2]
    g = geometry(f)
    M, N, K, batch = g.M, g.N, g.K, g.batch
    conv = kw.get("conv")
    geglu = kw.get("geglu") or 0
    Bm = _strided(B, (batch, N, K), (kw.get("strideB") or 0, _ld(B), 1)).double()
    if conv is None:
        lda = kw.get("lda") if kw.get("lda") is not None else _ld(A)
        Am = _strided(A, (batch, M, K), (kw.get("strideA") or 0, lda, 1)).double()
    else:
        assert batch == 1 and K == 9 * int(conv["Ci"])
        Am = im2col(A, conv, M).view(1, M, K)
    x = float(kw.get("alpha", 1.0)) * (Am @ Bm.transpose(1, 2))  # [batch, M, N]
    if kw.get("bias") is not None:
        x = x + _strided(kw["bias"], (N,), (1,)).double()
    x = act(x, kw.get("act") or 0)
    if kw.get("rowadd") is not None:
        rpg = int(kw.get("rows_per_group") or 1)
        ra = kw["rowadd"]
        rows = torch.arange(M, device=x.device) // rpg
        x = x + _strided(ra, (int(rows[-1]) + 1, N), (_ld(ra), 1)).double()[rows]
    if kw.get("resid") is not None:
        r = kw["resid"]
        x = x + _strided(r, (batch, M, N), (kw.get("strideC") or 0, _ld(r), 1)).double()
    gate = kw.get("gate")
    out2 = None
    if geglu == 2:
        assert batch == 1 and gate is not None
        h, gg = geglu_split(_strided(gate, (M, 2 * N), (_ld(gate), 1)).double())
        d = x[0]
        x = geglu_join(d * act(gg, 3), d * h * act_grad(gg, 3)).view(1, M, 2 * N)
    elif gate is not None:
        assert batch == 1
        x = x * act_grad(_strided(gate, (M, N), (_ld(gate), 1)).double(), int(kw["gate_act"]))
    if geglu == 1:
        h, gg = geglu_split(x[0])
        out2 = h * act(gg, 3)
    elif kw.get("out2") is not None:
        out2 = act(x[0], kw.get("act2") or 0)
    gn = None
    if kw.get("gn_sums") is not None:
        gn = gn_sums(x[0], int(kw["gn_hw"]), int(kw["gn_groups"]))
    return Ref(x if batch > 1 else x[0], out2, gn)
