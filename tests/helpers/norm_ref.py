"""Float64 references, input generators and the shape lists of the norm-kernel edge tests (tests/test_norm_edges_gpu.py,
tests/test_norm_ref_cpu.py).  Importing this touches no GPU.

References: plain float64 formulas written out here (not torch's own norms: tests/test_norm_ref_cpu.py compares them with
`F.group_norm` / `F.layer_norm` / `torch.softmax` in double), evaluated on whatever the caller passes — the GPU tests pass
the 16-bit-rounded tensors the kernel gets.  Activations are channels-last, `[Bn, HW, C]`, as the kernels see them.

Generators: `group_data` gives every (sample, group) its own mean and spread, so that a channel normalised with a
neighbouring group's statistics is wrong by O(1), not by 1 / sqrt(HW * cpg) as with identically distributed groups; with
`ratio` every group's mean dominates its spread by that factor (the case in which E[x^2] - E[x]^2 from f32 partial sums loses
digits).

`slab_emulation` replays the summation order of the slab statistics kernel (csrc/norms.hip gn_stats_kernel) in numpy.  It
predicts, it is no bar: nothing about a kernel is asserted from it."""
import functools

import numpy as np
import torch

# (Bn, HW, C, G) of the GroupNorm geometry cases; what each one reaches is said in tests/test_norm_edges_gpu.py
GN_EDGE_SHAPES = [
    (2, 64, 128, 32), (2, 50, 192, 32), (2, 50, 224, 32), (2, 36, 96, 8), (1, 81, 320, 32), (2, 108, 640, 32),
    (2, 7, 256, 64), (2, 2560, 256, 32), (2, 2048, 320, 32), (2, 2048, 256, 32), (2, 2049, 256, 32), (2, 16, 4096, 32),
    (2, 16, 4160, 32), (1, 5, 8320, 64),
]
GN_RATIO_SHAPE = (2, 256, 320, 32)     # the offset-dominated case
GN_RATIOS = [16, 64, 128, 256]         # 64 is asserted; the others are measured and printed
GN_REFUSED = {"cpg5": (2, 36, 160, 32), "cpg2": (2, 36, 64, 32), "G65": (2, 36, 520, 65), "C%8": (2, 36, 36, 4),
              "C%G": (2, 36, 320, 48)}

MEANS = (0.0, 1.0, -2.0, 4.0)
STDS = (0.25, 0.5, 1.0, 2.0)
RATIO_STD = 0.25
RATIO_SIZES = (1.0, 0.75, 1.25)        # |mean| = ratio * RATIO_STD * size


def group_stats(Bn, G, ratio=None):
    """the (mean, std) `group_data` aims at, each [Bn, G] float64.  No ratio: mean = MEANS[(g + 1) % 4], std = STDS[(g + b) % 4]
    — neighbouring groups differ by >= 1 in mean, no group's mean is more than 4 of its stds, and group 1 lies BELOW
    group 0 in every sample, so that a channel of group 0 taken for one of group 1 comes out large and positive and a SiLU
    behind the norm cannot squash the error.  ratio = r: std 0.25, mean
    = (-1)^g * 0.25 r * RATIO_SIZES[(g + b) % 3]."""
    g = torch.arange(G).reshape(1, G)
    b = torch.arange(Bn).reshape(Bn, 1)
    if ratio is None:
        mean = torch.tensor(MEANS, dtype=torch.float64)[(g + 1) % 4].expand(Bn, G)
        std = torch.tensor(STDS, dtype=torch.float64)[(g + b) % 4]
    else:
        sign = 1.0 - 2.0 * (g % 2).double()
        mean = sign * ratio * RATIO_STD * torch.tensor(RATIO_SIZES, dtype=torch.float64)[(g + b) % 3]
        std = torch.full((Bn, G), RATIO_STD, dtype=torch.float64)
    return mean.clone(), std.clone()


def group_data(Bn, HW, C, G, ratio=None, seed=0):
    """[Bn, HW, C] float32, group (b, g) drawn as mean + std * N(0, 1) with the statistics of `group_stats`; the caller
    rounds it to its 16-bit format"""
    gen = torch.Generator().manual_seed(seed)
    mean, std = group_stats(Bn, G, ratio)
    z = torch.randn(Bn, HW, G, C // G, generator=gen, dtype=torch.float64)
    x = mean.reshape(Bn, 1, G, 1) + std.reshape(Bn, 1, G, 1) * z
    return x.reshape(Bn, HW, C).float()


def achieved_ratio(x, G):
    """|mean| / std of every (sample, group) of x [Bn, HW, C], in float64 -> [Bn, G]"""
    Bn, HW, C = x.shape
    xg = x.double().reshape(Bn, HW, G, C // G)
    return xg.mean((1, 3)).abs() / xg.var((1, 3), unbiased=False).sqrt()


def gn_affine(C, seed=20):
    """gamma, beta as tests/test_kernels_gpu.py draws them (f32)"""
    g = torch.Generator().manual_seed(seed)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    g = torch.Generator().manual_seed(seed + 1)
    beta = 0.1 * torch.randn(C, generator=g)
    return gamma, beta


def _silu(v):
    return v * torch.sigmoid(v)


def groupnorm_ref(x, gamma, beta, G, eps, silu, dy=None, dtype=torch.float64):
    """x [Bn, HW, C] -> dict(y [Bn, HW, C], mean [Bn, G], rstd [Bn, G], dx [Bn, HW, C] if dy is given), all in `dtype`
    (float64: the reference; float32: the second evaluation `helpers.checks.check32` asks for)"""
    Bn, HW, C = x.shape
    xd = x.to(dtype).clone().requires_grad_(dy is not None)
    xg = xd.reshape(Bn, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    y = ((xg - mean) * rstd).reshape(Bn, HW, C) * gamma.to(dtype) + beta.to(dtype)
    if silu:
        y = _silu(y)
    out = {"y": y.detach(), "mean": mean.detach().reshape(Bn, G), "rstd": rstd.detach().reshape(Bn, G)}
    if dy is not None:
        y.backward(dy.to(dtype))
        out["dx"] = xd.grad
    return out


def layernorm_ref(x, gamma, beta, eps, dy=None, dtype=torch.float64):
    """x [rows, C] -> dict(y, mean [rows], rstd [rows], dx if dy is given), all in `dtype`"""
    xd = x.to(dtype).clone().requires_grad_(dy is not None)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = (xd - mean) * rstd * gamma.to(dtype) + beta.to(dtype)
    out = {"y": y.detach(), "mean": mean.detach().reshape(-1), "rstd": rstd.detach().reshape(-1)}
    if dy is not None:
        y.backward(dy.to(dtype))
        out["dx"] = xd.grad
    return out


def softmax_ref(x):
    """row softmax of x [rows, cols] in float64"""
    xd = x.double()
    e = torch.exp(xd - xd.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def misassign(y, x, gamma, beta, G, eps, silu):
    """the reference y [Bn, HW, C] with ONE channel wrong: the last channel of group 0 normalised with group 1's mean and
    rstd (what an off-by-one in a chunk's lo / hi split does) -> float64"""
    Bn, HW, C = x.shape
    cpg = C // G
    xg = x.double().reshape(Bn, HW, G, cpg)
    m1 = xg[:, :, 1].mean((1, 2)).reshape(Bn, 1)
    r1 = (xg[:, :, 1].var((1, 2), unbiased=False) + eps).rsqrt().reshape(Bn, 1)
    c = cpg - 1
    v = (x[:, :, c].double() - m1) * r1 * gamma[c].double() + beta[c].double()
    bad = y.double().clone()
    bad[:, :, c] = _silu(v) if silu else v
    return bad


def elem_excess(got, ref, tol, elem_k=8.0):
    """the largest |got - ref| over the allowance elem_k * tol * (rms(ref) + |ref|) of `helpers.checks.check`"""
    a, b = got.double(), ref.double()
    rms = b.pow(2).mean().sqrt()
    return ((a - b).abs() / (elem_k * tol * (rms + b.abs()))).max().item()


# ------------------------------------------------------------------------------------------ the slab path, emulated
def gn_geometry(HW, C):
    """TX, TY, rows per slab and slabs of csrc/norms.hip gn_geom"""
    CC = C // 8
    TX = min(CC, 256)
    TY = 256 // TX
    rps = max(8192 // C, 1)
    rps = (rps + TY - 1) // TY * TY
    nslab = (HW + rps - 1) // rps
    while nslab > 256:
        rps *= 2
        nslab = (HW + rps - 1) // rps
    return TX, TY, rps, nslab


def slab_emulation(x, G, eps, slab_totals_f32=True):
    """mean, rstd [Bn, G] (float64 arrays of the f32 results) as the slab statistics path forms them from x [Bn, HW, C]:
    thread (chunk, ty) of a slab walks the rows ty, ty + TY, ... of its `rps` rows and adds the 8 values of its chunk, in
    order, to f32 (sum, sum of squares) partials — one pair for the chunk's first group (lo) and one for its second (hi);
    the partials of a slab are added exactly (fixed point), the slab totals rounded to f32 (the three-launch form;
    `slab_totals_f32=False`: the two-launch form keeps them exact), the totals over the slabs formed in f64, and
    mean, var = E[x^2] - mean^2 in f64, var rounded to f32 before the reciprocal square root.  The square is rounded before
    it is added (the compiler may fuse the two: this is the pessimistic order)."""
    xs = x.detach().cpu().float().numpy()
    Bn, HW, C = xs.shape
    cpg, CC = C // G, C // 8
    _, TY, rps, nslab = gn_geometry(HW, C)
    ch0 = np.arange(CC) * 8
    g0 = ch0 // cpg
    split = (g0 + 1) * cpg - ch0
    S = np.zeros((Bn, G, 2), dtype=np.float64)
    for b in range(Bn):
        for s in range(nslab):
            r0, r1 = s * rps, min((s + 1) * rps, HW)
            lo = np.zeros((2, TY, CC), dtype=np.float32)
            hi = np.zeros((2, TY, CC), dtype=np.float32)
            for ty in range(TY):
                for r in range(r0 + ty, r1, TY):
                    row = xs[b, r].reshape(CC, 8)
                    for j in range(8):
                        v = row[:, j]
                        q = (v * v).astype(np.float32)
                        in_lo = j < split
                        lo[0, ty] = (lo[0, ty] + np.where(in_lo, v, np.float32(0))).astype(np.float32)
                        lo[1, ty] = (lo[1, ty] + np.where(in_lo, q, np.float32(0))).astype(np.float32)
                        hi[0, ty] = (hi[0, ty] + np.where(in_lo, np.float32(0), v)).astype(np.float32)
                        hi[1, ty] = (hi[1, ty] + np.where(in_lo, np.float32(0), q)).astype(np.float32)
            tot = np.zeros((G, 2), dtype=np.float64)
            for k in range(2):
                np.add.at(tot[:, k], g0, lo[k].astype(np.float64).sum(0))
                has_hi = split < 8
                np.add.at(tot[:, k], (g0 + 1)[has_hi], hi[k].astype(np.float64).sum(0)[has_hi])
            S[b] += tot.astype(np.float32).astype(np.float64) if slab_totals_f32 else tot
    inv_n = 1.0 / (HW * cpg)
    mu = S[..., 0] * inv_n
    var = np.maximum((S[..., 1] * inv_n - mu * mu).astype(np.float32), np.float32(0)) + np.float32(eps)
    rstd = (np.float32(1) / np.sqrt(var.astype(np.float64))).astype(np.float32)
    return mu.astype(np.float32).astype(np.float64), rstd.astype(np.float64)


def slab_prediction(x, gamma, beta, G, eps):
    """relative Frobenius errors (y, mean, rstd) the emulated slab statistics give against float64 on x; y is the f64
    apply with the emulated statistics, so the 16-bit rounding of the store is not in it"""
    Bn, HW, C = x.shape
    ref = groupnorm_ref(x, gamma, beta, G, eps, False)
    m, r = slab_emulation(x, G, eps)
    m, r = torch.from_numpy(m), torch.from_numpy(r)
    xg = x.double().reshape(Bn, HW, G, C // G)
    y = ((xg - m.reshape(Bn, 1, G, 1)) * r.reshape(Bn, 1, G, 1)).reshape(Bn, HW, C) * gamma.double() + beta.double()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    return rel(y, ref["y"]), rel(m, ref["mean"]), rel(r, ref["rstd"])


@functools.lru_cache(maxsize=None)
def gn_case(shape, silu, dt, ratio=None):
    """inputs (x, dy, accum in the 16-bit format `dt`; gamma, beta f32) of a GroupNorm case and its float64 and float32
    references, computed once per (shape, silu, format, ratio) and shared: treat every tensor as read-only"""
    Bn, HW, C, G = shape
    x = group_data(Bn, HW, C, G, ratio=ratio, seed=19).to(dt)
    gamma, beta = gn_affine(C)
    g = torch.Generator().manual_seed(22)
    dy = torch.randn(Bn, HW, C, generator=g).to(dt)
    g = torch.Generator().manual_seed(23)
    acc = torch.randn(Bn, HW, C, generator=g).to(dt)
    ref = groupnorm_ref(x, gamma, beta, G, 1e-5, silu, dy=dy)
    ref32 = groupnorm_ref(x, gamma, beta, G, 1e-5, silu, dtype=torch.float32)
    return {"x": x, "dy": dy, "acc": acc, "gamma": gamma, "beta": beta, "ref": ref, "ref32": ref32}
