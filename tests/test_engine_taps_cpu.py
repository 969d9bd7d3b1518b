"""The tests of the engine parity tests (no GPU): the proof that the loud-weight cases of tests/helpers/engine_taps.py are
sharp, and the record of how blind the plain synth weights are.

Sharp means: for EVERY 1-D tensor of a model's state dict, replacing it by zeros (a `.bias`) / ones (a gain) — what an
engine computes that drops the operand — and rolling it by one element — what an engine computes that mis-indexes it —
moves at least one quantity the GPU tests assert (a named tap or the end result) by at least twice that quantity's bar.
The bars are imported from the helper the GPU tests use.  Tensors the function is mathematically invariant to are listed
below with the reason, and the invariance of the end result is asserted; since the q/k/v projections are tapped, even those
are seen at a tap, so nothing is exempt."""
import re

import pytest
import torch

from helpers import engine_taps as ET
from helpers import loud_weights as LW

MARGIN = 2.0

# name pattern -> why the function does not depend on the tensor
INVARIANT = {
    r"self_attn\.k_proj\.bias$": "adds q.b, the same constant, to every key's score of a query: softmax removes it",
    r"mid_block\.attentions\.0\.key\.bias$": "single-head attention: the same constant on every key's score of a query",
}

MODELS = {
    "unet-tiny": ("unet", lambda: ET.unet_case("tiny", 1, 8, 16), ET.unet_oracle),
    "unet-tiny21": ("unet", lambda: ET.unet_case("tiny21", 1, 8, 16), ET.unet_oracle),
    "vae-encoder": ("vae_enc", lambda: ET.vae_enc_case(1, 64, 64), ET.vae_enc_oracle),
    "vae-decoder": ("vae_dec", lambda: ET.vae_dec_case(1, 8, 8), ET.vae_dec_oracle),
    "clip-tiny": ("text", lambda: ET.clip_case("tiny"), ET.clip_oracle),
    "clip-tiny21": ("text", lambda: ET.clip_case("tiny21"), ET.clip_oracle),
}


def test_loud_is_pure_and_overrides_only_1d():
    cfg, w, _ = ET.vae_dec_case(1, 8, 8, loud_seed=None)
    before = {k: v.clone() for k, v in w.items()}
    a, b, c = LW.loud(w, 3), LW.loud(w, 3), LW.loud(w, 4)
    assert all(torch.equal(w[k], before[k]) for k in w), "the argument was modified"
    assert all(torch.equal(a[k], b[k]) for k in w) and list(a) == list(w)
    for k, v in w.items():
        if v.dim() == 1:
            assert not torch.equal(a[k], c[k]) and torch.equal(a[k], a[k].half().float())
        else:
            assert a[k] is v
    bias = torch.cat([a[k] for k in w if w[k].dim() == 1 and k.endswith(".bias")])
    gain = torch.cat([a[k] for k in w if w[k].dim() == 1 and not k.endswith(".bias")])
    print(f"loud: {bias.numel()} bias elements std {bias.std():.3f}; {gain.numel()} gain elements in "
          f"[{gain.min():.3f}, {gain.max():.3f}]")
    assert abs(bias.std() - LW.BIAS_STD) < 0.02 and abs(bias.mean()) < 0.02
    assert gain.min() >= 1 - LW.GAIN_HALF_WIDTH and gain.max() <= 1 + LW.GAIN_HALF_WIDTH and gain.std() > 0.25


def test_taps_change_nothing_and_golden_calls_are_bit_identical():
    """a call with taps returns the bits of a call without"""
    from oracle import sd_ref as R
    cfg, w, inp = ET.unet_case("tiny21", 1, 8, 16)
    with torch.no_grad():
        ctx = lambda: dict({f"CONTEXT_TENSOR_{i}": inp["ck"][i].float().view(1, 77, -1) for i in range(16)}, this_idx=0)
        taps = {}
        assert torch.equal(R.unet_forward(w, cfg, inp["x"], inp["t"], ctx()),
                           R.unet_forward(w, cfg, inp["x"], inp["t"], ctx(), taps))
        assert len(taps) > 100 and all(not t.requires_grad for t in taps.values())
        cfg, w, x = ET.vae_enc_case(1, 64, 64)
        assert torch.equal(R.vae_encode_moments(w, cfg, x.half().float()), ET.vae_enc_oracle(cfg, w, x)["end"])
        cfg, w, z = ET.vae_dec_case(1, 8, 8)
        assert torch.equal(R.vae_decode(w, cfg, z / cfg.scaling_factor), ET.vae_dec_oracle(cfg, w, z)["end"])


@pytest.mark.parametrize("model", list(MODELS))
def test_every_1d_tensor_is_visible_at_twice_a_bar(model):
    family, case, oracle = MODELS[model]
    cfg, w, inp = case()
    base = oracle(cfg, w, inp)
    names = LW.names_1d(w)
    weakest, weakest_at, n_inv, failures = float("inf"), None, 0, []
    for name in names:
        for how, mutate in (("dropped", LW.drop), ("rolled", LW.roll)):
            mut = oracle(cfg, mutate(w, name), inp)
            why = [r for p, r in INVARIANT.items() if re.search(p, name)]
            if why:
                moved = ET.rel(mut["end"], base["end"])
                assert moved < 1e-5, f"{model}: {name} {how} is listed as invariant ({why[0]}) but moves the output by {moved:.2e}"
                n_inv += 1  # (the q/k/v tap still sees the operand itself: no exemption from the bars below)
            s, where = ET.strongest(family, base, mut)
            if s < weakest:
                weakest, weakest_at = s, f"{name} {how} (seen at {where})"
            if s < MARGIN:
                failures.append(f"{name} {how}: best signal {s:.2f} x its bar, at {where}")
    print(f"[{model}] {len(names)} 1-D tensors, {len(base) - 1} taps, 2 mutations each; {n_inv // 2} invariant; weakest margin "
          f"{weakest:.2f} x the bar: {weakest_at}")
    assert not failures, f"{model}: {len(failures)} mutations no asserted quantity sees at {MARGIN} x its bar:\n" + "\n".join(failures)


def test_plain_synth_weights_are_blind():
    """the recorded fact behind the loud weights: on plain synth weights, at the bars tests/test_unet_gpu.py always had
    (pred 2e-2, worst context gradient 4e-2; tiny, B=1, 8x16), dropping one 1-D tensor goes unnoticed for more than half of
    them (399 of 404 when this was written), and on the VAE encoder (1x64x64, 1e-2) for 53 of 75"""
    cfg, w, inp = ET.unet_case("tiny", 1, 8, 16, loud_seed=None)
    base, leaves = ET.unet_oracle(cfg, w, inp, grads=True)
    g0 = [t.grad for ab in leaves for t in ab]
    names = LW.names_1d(w)
    blind = 0
    for name in names:
        mut, lv = ET.unet_oracle(cfg, LW.drop(w, name), inp, grads=True)
        e_pred = ET.rel(mut["end"], base["end"])
        e_grad = max(ET.rel(t.grad, g) for t, g in zip((t for ab in lv for t in ab), g0))
        blind += e_pred < ET.END["unet"] and e_grad < ET.END["unet.grad"]
    cfg, w, x = ET.vae_enc_case(1, 64, 64, loud_seed=None)
    vbase = ET.vae_enc_oracle(cfg, w, x)["end"]
    vnames = LW.names_1d(w)
    vblind = sum(ET.rel(ET.vae_enc_oracle(cfg, LW.drop(w, n), x)["end"], vbase) < ET.END["vae_enc"] for n in vnames)
    print(f"[synth] UNet: {blind} of {len(names)} 1-D tensors dropped without the end-to-end bars noticing; "
          f"VAE encoder: {vblind} of {len(vnames)}")
    assert blind > len(names) // 2
