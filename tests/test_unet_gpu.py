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


@pytest.mark.parametrize("cfg_name,B,H,W", [("tiny", 2, 16, 16), ("tiny", 1, 8, 16), ("tiny21", 2, 16, 16), ("tiny21", 1, 8, 16)])
def test_unet_loud_weights_and_taps(cfg_name, B, H, W):
    """The same comparison on LOUD 1-D parameters (helpers/loud_weights.py: a dropped, swapped or mis-indexed bias, gain or
    shift moves the result by many bars; tests/test_engine_taps_cpu.py proves it for every 1-D tensor), at the same
    end-to-end bars, and every named tap of the oracle against the engine buffer that holds it (helpers/engine_taps.py,
    which states the measured tap errors and their bars).  tiny21 runs the linear proj_in / proj_out form.  fp16 library
    only: `t16` would widen bf16 bars eightfold, which leaves the sharpness proof no margin; bf16 keeps its whole-step check.
    Measured on an MI355X (fp16): pred 1.2e-3 (bar 2e-2), worst context gradient 4.2e-3 (bar 4e-2); worst tap error per
    kind, over these cases and the UNets of the loud whole steps: time 4.2e-4 (bar 9e-4), every other kind (conv, res.gn,
    res.h1, res.out, tr.gn, tr.ln, tr.h0, tr.h1, tr.h2, tr.out, head.gn) 1.2e-3 .. 1.5e-3 (bar 3e-3 = 2 x the worst, rounded
    up); TAP["unet"] in helpers/engine_taps.py lists each."""
    from helpers import engine_taps as ET
    from helpers.checks import DT
    from view_neti_amd.engine.unet import UNetEngine
    if DT != torch.float16:
        pytest.skip("engine taps are measured and proven for the fp16 library")
    cfg, w, inp = ET.unet_case(cfg_name, B, H, W)
    eng = UNetEngine(cfg, w, B, H, W)
    eng.x_in.copy_(inp["x"])
    eng.timesteps.copy_(inp["t"])
    eng.ctx_k.copy_(inp["ck"])
    eng.ctx_v.copy_(inp["cv"])
    eng.forward()
    torch.cuda.synchronize()
    ref, leaves = ET.unet_oracle(cfg, w, inp, grads=True)
    label = f"unet loud {cfg_name} {B}x{H}x{W}"
    pred = eng.pred.float().cpu().view(B, H, W, 4).permute(0, 3, 1, 2)
    e = _rel(pred, ref["end"])
    print(f"[{label}] pred rel err {e:.3e} (ref std {ref['end'].std().item():.3f})")
    ET.compare(label, "unet", {k: v for k, v in ref.items() if k != "end"}, ET.unet_buffers(eng), ET.norm_outputs(eng))
    assert math.isfinite(e) and e < ET.END["unet"]
    eng.dpred.copy_(inp["dpred"].permute(0, 2, 3, 1).reshape(B * H * W, 4))
    eng.backward()
    torch.cuda.synchronize()
    L, Dc = inp["L"], cfg.cross_attention_dim
    worst = max(max(_rel(eng.dctx_k[i].view(B, L, Dc), a.grad), _rel(eng.dctx_v[i].view(B, L, Dc), b.grad))
                for i, (a, b) in enumerate(leaves))
    print(f"[{label}] worst context-gradient rel err {worst:.3e}")
    assert math.isfinite(worst) and worst < ET.END["unet.grad"]
