"""VAE encoder engine vs the CPU oracle (moments = quant_conv(encoder(x)))."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 64, 128)])
def test_vae_encoder_tiny(B, H, W):
    from oracle import sd_ref as R
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.vae import VAEEncoderEngine
    cfg = sc.tiny().vae
    w = {k: v.half().float() for k, v in synth.vae_weights(cfg).items()}
    eng = VAEEncoderEngine(cfg, w, B, H, W)
    x = synth.pixel_values(B, H, W)
    eng.x_in.copy_(x)
    eng.forward()
    torch.cuda.synchronize()
    got = eng.moments.float().cpu().view(B, H // 8, W // 8, 8).permute(0, 3, 1, 2)
    ref = R.vae_encode_moments(w, cfg, x.half().float())
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"[vae tiny {B}x{H}x{W}] moments rel err {rel:.3e} (ref std {ref.std():.3f}), {len(eng.fwd)} launches")
    assert math.isfinite(rel) and rel < 1e-2


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 64, 128)])
def test_vae_encoder_loud_weights_and_taps(B, H, W):
    """The same comparison on LOUD 1-D parameters (helpers/loud_weights.py), at the same end-to-end bar, and every named tap
    of the oracle — conv_in, each ResNet's two GroupNorm-SiLU outputs, h1 and out, the downsamplers, the mid attention's
    GroupNorm, q/k/v projection and output, the head's norm — against the engine buffer that holds it.
    Measured on an MI355X (fp16): moments 1.1e-3 (bar 1e-2); worst tap error per kind: conv 9.1e-4 (bar 2e-3), res.gn,
    res.h1, res.out, attn.gn, attn.qkv, attn.out, head.gn 1.0e-3 .. 1.2e-3 (bar 3e-3 = 2 x the worst, rounded up); TAP["vae_enc"]
    in helpers/engine_taps.py lists each.  tests/test_engine_taps_cpu.py
    proves that every dropped or mis-indexed 1-D tensor moves one of these quantities by twice its bar.  fp16 library only:
    `t16` would widen bf16 bars eightfold, which leaves that proof no margin."""
    from helpers import engine_taps as ET
    from helpers.checks import DT
    from view_neti_amd.engine.vae import VAEEncoderEngine
    if DT != torch.float16:
        pytest.skip("engine taps are measured and proven for the fp16 library")
    cfg, w, x = ET.vae_enc_case(B, H, W)
    eng = VAEEncoderEngine(cfg, w, B, H, W)
    eng.x_in.copy_(x)
    eng.forward()
    torch.cuda.synchronize()
    ref = ET.vae_enc_oracle(cfg, w, x)
    label = f"vae loud {B}x{H}x{W}"
    got = eng.moments.float().cpu().view(B, H // 8, W // 8, 8).permute(0, 3, 1, 2)
    rel = ET.rel(got, ref["end"])
    print(f"[{label}] moments rel err {rel:.3e} (ref std {ref['end'].std():.3f})")
    ET.compare(label, "vae_enc", {k: v for k, v in ref.items() if k != "end"}, ET.vae_buffers(eng), ET.norm_outputs(eng))
    assert math.isfinite(rel) and rel < ET.END["vae_enc"]


def test_vae_taps_refuse_an_engine_that_misreads_one_shift():
    """the tap comparison really reads the engine: an engine built on weights in which ONE GroupNorm shift is rolled by one
    element (the oracle keeps the right ones) is refused, the ResNet GroupNorm outputs among the kinds named"""
    from helpers import engine_taps as ET
    from helpers import loud_weights as LW
    from helpers.checks import DT
    from view_neti_amd.engine.vae import VAEEncoderEngine
    if DT != torch.float16:
        pytest.skip("engine taps are measured and proven for the fp16 library")
    B, H, W = 1, 64, 64
    cfg, w, x = ET.vae_enc_case(B, H, W)
    eng = VAEEncoderEngine(cfg, LW.roll(w, "encoder.down_blocks.1.resnets.0.norm2.bias"), B, H, W)
    eng.x_in.copy_(x)
    eng.forward()
    torch.cuda.synchronize()
    ref = ET.vae_enc_oracle(cfg, w, x)
    with pytest.raises(AssertionError, match="taps beyond their bars") as exc:
        ET.compare("vae misread shift", "vae_enc", {k: v for k, v in ref.items() if k != "end"}, ET.vae_buffers(eng),
                   ET.norm_outputs(eng))
    assert "res.gn" in str(exc.value)
