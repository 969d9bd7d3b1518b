"""UNet engine (HIP schedule) vs the CPU oracle: predicted noise and the 32 context gradients.
Weights/inputs are rounded to f16 once so both sides see identical values; tolerances cover f16
activation storage through ~130 kernels (fp32 oracle)."""
import math

import pytest
import torch

from helpers.checks import frob_rel as _rel

pytestmark = pytest.mark.gpu


def _run(cfg_name, B, H, W, tol_pred, tol_grad):
    from oracle import sd_ref as R
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.unet import UNetEngine
    cfg = sc.CONFIGS[cfg_name]().unet
    w = {k: v.half().float() for k, v in synth.unet_weights(cfg).items()}
    eng = UNetEngine(cfg, w, B, H, W)
    L, Dc, nl = 77, cfg.cross_attention_dim, cfg.n_cross_layers
    x = synth.gaussian((B, 4, H, W), 5)
    t = synth.timesteps(B)
    ck = synth.gaussian((nl, B * L, Dc), 6).half()
    cv = synth.gaussian((nl, B * L, Dc), 7).half()
    dpred = synth.gaussian((B, 4, H, W), 8).half()
    eng.x_in.copy_(x)
    eng.timesteps.copy_(t)
    eng.ctx_k.copy_(ck)
    eng.ctx_v.copy_(cv)
    eng.forward()
    torch.cuda.synchronize()
    pred = eng.pred.float().cpu().view(B, H, W, 4).permute(0, 3, 1, 2)
    # oracle
    ctx = {"this_idx": 0}
    leaves = []
    for i in range(nl):
        a = ck[i].float().view(B, L, Dc).requires_grad_(True)
        b = cv[i].float().view(B, L, Dc).requires_grad_(True)
        ctx[f"CONTEXT_TENSOR_{i}"] = a
        ctx[f"CONTEXT_TENSOR_BYPASS_{i}"] = b
        leaves.append((a, b))
    ref = R.unet_forward(w, cfg, x, t, ctx)
    e = _rel(pred, ref.detach())
    print(f"[unet {cfg_name}] pred rel err {e:.3e}  (ref std {ref.std().item():.3f})")
    assert math.isfinite(e) and e < tol_pred
    (ref * dpred.float()).sum().backward()
    eng.dpred.copy_(dpred.permute(0, 2, 3, 1).reshape(B * H * W, 4))
    eng.backward()
    torch.cuda.synchronize()
    worst = 0.0
    for i, (a, b) in enumerate(leaves):
        ek = _rel(eng.dctx_k[i].view(B, L, Dc), a.grad)
        ev = _rel(eng.dctx_v[i].view(B, L, Dc), b.grad)
        print(f"[unet {cfg_name}] layer {i:2d} dctx_k rel {ek:.3e} (|g| {a.grad.norm():.3e})  dctx_v rel {ev:.3e}")
        worst = max(worst, ek, ev)
    assert math.isfinite(worst) and worst < tol_grad
    print(f"[unet {cfg_name}] engine memory {eng.bytes / 2**20:.1f} MiB, {len(eng.fwd)} fwd + {len(eng.bwd)} bwd launches")


def test_unet_tiny_fwd_bwd():
    _run("tiny", 2, 16, 16, 2e-2, 4e-2)


def test_unet_tiny_nonsquare():
    _run("tiny", 1, 8, 16, 2e-2, 4e-2)
