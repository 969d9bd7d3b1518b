"""The tolerance rules of the GPU suite, stated once: the 16-bit format of the process and its bf16 factor (`t16`; the
docstring of tests/test_kernels_gpu.py explains the factor), the two-bound `check`, the f32 bar rule `check32`, and the
small generators every kernel file uses.  Importing this touches no GPU (`ops()` is lazy).

The f32 bar rule (`check32`): an f32 output with no 16-bit rounding between the shared inputs and it is held to 1e-5 where
plain f32 arithmetic can meet that; the check also evaluates its reference in torch float32 on the CPU, e32 = that result's
relative Frobenius error against float64, and the bar is 1e-5 if 8 * e32 <= 1e-5, else 8 * e32.  No bar comes from a
kernel's output.

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import math

import torch

from view_neti_amd import lib as _lib  # (ctypes only: importing it loads no library and touches no GPU)

DEV = "cuda"
DT = _lib.act_dtype()                         # torch.float16, or torch.bfloat16 under VNETI_PRECISION=bf16
TOL16 = 8.0 if DT == torch.bfloat16 else 1.0  # unit roundoff of DT over fp16's


def t16(tol):
    """the tolerance of a check through a 16-bit store: the stated fp16 number, times 8 in bf16"""
    return tol * TOL16


def ops():
    from view_neti_amd import ops
    return ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, scale=1.0, seed=0, dtype=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DT if dtype is None else dtype)


def relerr(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item(), (a - b).abs().max().item()


ELEM_K = 8.0


def check(name, got, ref, tol, elem_k=ELEM_K):
    """two bounds: the relative Frobenius norm (< tol), and an ELEMENT-WISE one so that a wrong tail row / column of a
    large output cannot hide inside the norm: |got - ref| <= elem_k * tol * (rms(ref) + |ref|) for every element
    (f16 rounding scales with the element, accumulation noise with the tensor's rms; a Gaussian error of sigma =
    tol * rms stays under 6 sigma over 1e7 elements, a dropped or misplaced element is off by ~|ref| itself)."""
    a, b = got.float().cpu(), ref.float().cpu()
    r, m = relerr(a, b)
    rms = b.pow(2).mean().sqrt()
    excess = (a - b).abs() - elem_k * tol * (rms + b.abs())
    worst = excess.max().item()
    print(f"[{name}] rel={r:.3e} maxabs={m:.3e} elem-bound margin={-worst:.3e}")
    assert math.isfinite(r) and r < tol, f"{name}: rel err {r} (max abs {m}) >= {tol}"
    if worst > 0:
        idx = [int(i) for i in torch.unravel_index(excess.argmax(), excess.shape)]
        raise AssertionError(f"{name}: element {idx} off by {(a - b)[tuple(idx)].item():.4e} (ref {b[tuple(idx)].item():.4e}, "
                             f"rms {rms.item():.3e}): beyond the element-wise bound {elem_k}*{tol}*(rms+|ref|)")


F32_BAR = 1e-5


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def check32(name, got, ref64, ref32, floor=F32_BAR):
    """the f32 bar rule of the module docstring; prints e32, the kernel's error and the bar"""
    e32 = rel(ref32, ref64)
    bar = floor if 8 * e32 <= floor else 8 * e32
    print(f"[{name}] e32={e32:.3e} kernel={rel(got.cpu(), ref64):.3e} bar={bar:.3e}")
    check(name, got, ref64, bar)


def frob_rel(a, b):
    """relative Frobenius error in float32 on the host: the figure the engine-level files (text, unet, infer, nvs) bound"""
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def attn_ref(q, k, v, H, D, scale, causal):
    Bn, Nq, _ = q.shape
    Nk = k.shape[1]
    qh = q.view(Bn, Nq, H, D).transpose(1, 2)
    kh = k.view(Bn, Nk, H, D).transpose(1, 2)
    vh = v.view(Bn, Nk, H, D).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(Nq, Nk, dtype=torch.bool).tril()
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    o = (p @ vh).transpose(1, 2).reshape(Bn, Nq, H * D)
    lse = torch.logsumexp(s, -1)
    return o, lse
