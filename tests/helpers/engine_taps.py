"""Engine parity on loud weights, stated once for the GPU tests that assert it and the CPU proof that it is sharp
(tests/test_engine_taps_cpu.py): the cases (weights, inputs), the oracle runs with their named taps (oracle/sd_ref.py), the
bars, and the walk that finds in an engine the buffer behind every tap.  Importing this touches no GPU.

Every quantity is a relative Frobenius error against the fp32 oracle.  A tap belongs to a KIND (all GroupNorm-SiLU outputs
of ResNets are one kind, ...) and a kind has one bar per engine family.

The bars.  `END` are the end-to-end bars the engine files always had.  `TAP` were measured: the loud cases below were run
on an MI355X against the fp16 library, the worst error of each kind over all cases of the family was taken, doubled (the
run-to-run and box-to-box headroom of the suite's other measured bars) and rounded up to one digit; no tap bar may exceed
its family's end-to-end bar.  The measured values stand next to each bar.  These cases run against the fp16 library only:
`t16` widens bf16 bars eightfold, which would leave the sharpness proof no margin; bf16 keeps its whole-step check.

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import math

import torch

from helpers import loud_weights as LW

LOUD_SEED = 41

END = {"unet": 2e-2, "unet.grad": 4e-2, "vae_enc": 1e-2, "vae_dec": 5e-3, "text": 5e-3}

# kind -> bar                      # measured worst (MI355X, fp16 library; over the family's engine-level loud cases and the
TAP = {                            # sub-engines of the four loud whole-step cases)
    "unet": {"time": 9e-4,         # 4.172e-04
             "conv": 3e-3,         # 1.449e-03
             "res.gn": 3e-3,       # 1.416e-03
             "res.h1": 3e-3,       # 1.155e-03
             "res.out": 3e-3,      # 1.381e-03
             "tr.gn": 3e-3,        # 1.424e-03
             "tr.ln": 3e-3,        # 1.435e-03
             "tr.h0": 3e-3,        # 1.437e-03
             "tr.h1": 3e-3,        # 1.305e-03
             "tr.h2": 3e-3,        # 1.302e-03
             "tr.out": 3e-3,       # 1.385e-03
             "head.gn": 3e-3},     # 1.467e-03
    "vae_enc": {"conv": 2e-3,      # 9.094e-04
                "res.gn": 3e-3,    # 1.212e-03
                "res.h1": 3e-3,    # 1.099e-03
                "res.out": 3e-3,   # 1.046e-03
                "attn.gn": 3e-3,   # 1.084e-03
                "attn.qkv": 3e-3,  # 1.084e-03
                "attn.out": 3e-3,  # 1.007e-03
                "head.gn": 3e-3},  # 1.198e-03
    "vae_dec": {"conv": 3e-3,      # 1.054e-03
                "res.gn": 3e-3,    # 1.399e-03
                "res.h1": 3e-3,    # 1.200e-03
                "res.out": 3e-3,   # 1.147e-03
                "attn.gn": 1e-3,   # 4.683e-04
                "attn.qkv": 1e-3,  # 4.988e-04
                "attn.out": 1e-3,  # 4.993e-04
                "head.gn": 3e-3},  # 1.307e-03
    "text": {"ln": 9e-4,           # 4.026e-04
             "qkv": 9e-4,          # 4.323e-04
             "attn": 7e-4,         # 3.241e-04
             "mlp": 8e-4},         # 3.629e-04
}
for _fam, _bars in TAP.items():
    assert max(_bars.values()) <= END[_fam], f"{_fam}: a tap bar above the end-to-end bar"

GN_KINDS = ("res.gn", "tr.gn", "tr.ln", "attn.gn", "head.gn", "ln")  # found in the launch list, not on the tape


def kind(key):
    """the kind of an oracle tap, from its name"""
    leaf = key.rsplit(".", 1)[-1]
    if key.startswith("time."):
        return "time"
    if key.startswith("text_model."):
        return "ln" if leaf in ("ln1", "ln2") else leaf
    if key.endswith("conv_norm_out.y"):
        return "head.gn"
    if key.endswith("conv_in") or key == "post_quant_conv" or "samplers." in key:
        return "conv"
    if "mid_block.attentions" in key and key.split(".")[0] in ("encoder", "decoder"):
        return "attn." + leaf
    if ".attentions." in key:
        return "tr.ln" if leaf in ("ln1", "ln2", "ln3") else "tr." + leaf
    if ".resnets." in key:
        return "res.gn" if leaf in ("gn1", "gn2") else "res." + leaf
    raise KeyError(key)


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


# ---------------------------------------------------------------------------------------------------- cases and oracle runs
def r16(w):
    return {k: v.half().float() for k, v in w.items()}


def unet_case(cfg_name, B, H, W, loud_seed=LOUD_SEED):
    """-> cfg, weights (f16-rounded, loud unless loud_seed is None), inputs: the tensors of tests/test_unet_gpu.py"""
    from view_neti_amd import sd_config as sc, synth
    cfg = sc.CONFIGS[cfg_name]().unet
    w = r16(synth.unet_weights(cfg))
    if loud_seed is not None:
        w = LW.loud(w, loud_seed)
    L, Dc, nl = 77, cfg.cross_attention_dim, cfg.n_cross_layers
    inp = dict(x=synth.gaussian((B, 4, H, W), 5), t=synth.timesteps(B), ck=synth.gaussian((nl, B * L, Dc), 6).half(),
               cv=synth.gaussian((nl, B * L, Dc), 7).half(), dpred=synth.gaussian((B, 4, H, W), 8).half(), B=B, L=L)
    return cfg, w, inp


def unet_oracle(cfg, w, inp, grads=False):
    """-> {"end": pred, taps...} in call order (and the context-gradient leaves if grads)"""
    from oracle import sd_ref as R
    B, L, Dc, nl = inp["B"], inp["L"], cfg.cross_attention_dim, cfg.n_cross_layers
    ctx, leaves = {"this_idx": 0}, []
    for i in range(nl):
        a, b = inp["ck"][i].float().view(B, L, Dc), inp["cv"][i].float().view(B, L, Dc)
        if grads:
            a.requires_grad_(True), b.requires_grad_(True)
            leaves.append((a, b))
        ctx[f"CONTEXT_TENSOR_{i}"], ctx[f"CONTEXT_TENSOR_BYPASS_{i}"] = a, b
    taps = {}
    with torch.set_grad_enabled(grads):
        pred = R.unet_forward(w, cfg, inp["x"], inp["t"], ctx, taps)
    if grads:
        (pred * inp["dpred"].float()).sum().backward()
        return dict(taps, end=pred.detach()), leaves
    return dict(taps, end=pred)


def vae_enc_case(B, H, W, loud_seed=LOUD_SEED):
    from view_neti_amd import sd_config as sc, synth
    cfg = sc.tiny().vae
    w = r16(synth.vae_weights(cfg))
    if loud_seed is not None:
        w = LW.loud(w, loud_seed)
    return cfg, w, synth.pixel_values(B, H, W)


def vae_enc_oracle(cfg, w, x):
    from oracle import sd_ref as R
    taps = {}
    with torch.no_grad():
        end = R.vae_encode_moments(w, cfg, x.half().float(), taps)
    return dict(taps, end=end)


def vae_dec_case(B, h, w_, loud_seed=LOUD_SEED):
    """weights as tests/test_infer_gpu.py rounds them: the engine holds post_quant_conv and every 1-D tensor in f32"""
    from view_neti_amd import sd_config as sc, synth
    cfg = sc.tiny().vae
    wts = synth.vae_decoder_weights(cfg)
    w = {k: (v.half().float() if v.dim() >= 2 and not k.startswith("post_quant") else v) for k, v in wts.items()}
    if loud_seed is not None:
        w = LW.loud(w, loud_seed)
    return cfg, w, synth.gaussian((B, 4, h, w_), 21) * cfg.scaling_factor


def vae_dec_oracle(cfg, w, z):
    from oracle import sd_ref as R
    taps = {}
    with torch.no_grad():
        end = R.vae_decode(w, cfg, z / cfg.scaling_factor, taps)
    return dict(taps, end=end)


def clip_case(cfg_name, B=2, loud_seed=LOUD_SEED):
    """the CLIP stack alone (the proof's model of the text engine): plain ids, L = 77"""
    from view_neti_amd import sd_config as sc, synth
    cfg = sc.CONFIGS[cfg_name]().clip
    w = synth.clip_weights(cfg)
    w = {k: (v.half().float() if (k.endswith("weight") and v.dim() == 2 and "embedding" not in k) else v) for k, v in w.items()}
    if loud_seed is not None:
        w = LW.loud(w, loud_seed)
    ids = synth.input_ids(B, cfg.vocab_size - 3, cfg.vocab_size, cfg.max_positions)
    ids[1:] = torch.roll(ids[1:], 3, dims=1)
    return cfg, w, ids


def clip_oracle(cfg, w, ids):
    """end = the context the text engine writes: final_layer_norm of the last hidden state"""
    from oracle import sd_ref as R
    import torch.nn.functional as F
    taps = {}
    with torch.no_grad():
        x = R.neti_embeddings(w["text_model.embeddings.token_embedding.weight"],
                              w["text_model.embeddings.position_embedding.weight"], ids, None, None)
        last = R.clip_encoder(w, cfg, x, taps)
        end = F.layer_norm(last, (last.shape[-1],), w["text_model.final_layer_norm.weight"],
                           w["text_model.final_layer_norm.bias"], cfg.eps)
    return dict(taps, end=end)


def bar(family, key):
    return END[family] if key == "end" else TAP[family][kind(key)]


def strongest(family, base, mutated):
    """max over the asserted quantities of (how far the mutation moves it) / (its bar), and the quantity's name"""
    best, where = 0.0, None
    for key, ref in base.items():
        s = rel(mutated[key], ref) / bar(family, key)
        if s > best:
            best, where = s, key
    return best, where


# ---------------------------------------------------------------------------------------------------- the engine side
def _launches(eng, funcs):
    return [f for f in list(eng.fwd_pre) + list(eng.fwd) if getattr(f, "func", None) in funcs]


def norm_outputs(eng):
    """the output buffer of every GroupNorm / LayerNorm launch of the forward lists, in launch order (args: x, y, gamma, ...)"""
    from view_neti_amd import ops
    return [f.args[1] for f in _launches(eng, (ops.groupnorm_fwd, ops.groupnorm_fwd_2l, ops.groupnorm_fwd_sums,
                                               ops.layernorm_fwd))]


def _resnet_bufs(r):
    return [("res.h1", r["h1"].v), ("res.out", r["out"].v)]


def unet_buffers(eng):
    """[(kind, buffer)] of everything but the norm outputs, in tape order = oracle call order"""
    out = [("time", eng.t_sin), ("time", eng.t_h), ("time", eng.t_emb), ("conv", eng.tape[0]["x"].v)]
    for r in eng.tape:
        k = r["kind"]
        if k == "resnet":
            out += _resnet_bufs(r)
        elif k == "transformer":
            out += [("tr.h0", r["h0"]), ("tr.h1", r["h1"]), ("tr.h2", r["h2"]), ("tr.out", r["out"].v)]
        elif k in ("down", "up"):
            out.append(("conv", r["out"].v))
        else:
            assert k == "head", f"unknown tape record {k}"
    return out


def vae_buffers(eng):
    """the encoder or the decoder: neither records its mid attention nor the decoder its upsamplers; their outputs are the
    inputs (`x`) of the ResNet records that follow them"""
    from view_neti_amd import ops
    out = [("conv", f.args[3]) for f in _launches(eng, (ops.conv1x1_nchw,))]  # decoder: post_quant_conv (f32, NCHW)
    out.append(("conv", eng.tape[0]["x"].v))
    for r in eng.tape:
        if r["kind"] == "down":
            out.append(("conv", r["out"].v))
            continue
        assert r["kind"] == "resnet", f"unknown tape record {r['kind']}"
        if r["name"].endswith("mid_block.resnets.1."):
            # the mid attention's q/k/v projection: the one biased plain GEMM that reads a norm output and is 3 x as wide
            ys = {y.data_ptr() for y in norm_outputs(eng)}
            qkv = [f.args[2] for f in _launches(eng, (ops.gemm,)) if f.args[0].data_ptr() in ys and not f.keywords.get("conv")
                   and f.keywords.get("bias") is not None and f.args[2].shape[-1] == 3 * f.args[0].shape[-1]]
            assert len(qkv) == 1, f"{len(qkv)} candidates for the mid attention's q/k/v projection"
            out += [("attn.qkv", qkv[0]), ("attn.out", r["x"].v)]
        elif r["name"].startswith("decoder.up_blocks.") and r["name"].endswith(".resnets.0.") and \
                not r["name"].startswith("decoder.up_blocks.0."):
            out.append(("conv", r["x"].v))
        out += _resnet_bufs(r)
    return out


def text_buffers(eng):
    out = []
    for i, r in enumerate(eng.layers):
        out += [("qkv", r["qkv"]), ("attn", r["x_mid"])]
        out.append(("mlp", eng.layers[i + 1]["x_in"] if i + 1 < len(eng.layers) else eng.last))
    return out


def stack_text_taps(passes):
    """the per-pass tap dicts of R.text_conditioning -> one dict of (passes * B * L, D) tensors: the text engine's row order"""
    return {k: torch.cat([p[k].reshape(-1, p[k].shape[-1]) for p in passes]) for k in passes[0]}


def _as_rows(ref, got):
    """the oracle tensor in the layout of the engine buffer: channels-last rows (or NCHW as it is)"""
    if tuple(ref.shape) == tuple(got.shape):
        return ref
    if ref.dim() == 4:
        ref = ref.permute(0, 2, 3, 1)
    return ref.reshape(-1, ref.shape[-1])


def compare(label, family, taps, buffers, norms):
    """every oracle tap (`taps`: name -> tensor in call order, without "end") against the engine buffer that holds it, on
    the device; prints the worst error per kind, asserts every one against its bar; -> {kind: worst}"""
    keys = [k for k in taps if k != "end"]
    kn = [k for k in keys if kind(k) in GN_KINDS]
    kb = [k for k in keys if kind(k) not in GN_KINDS]
    assert len(kn) == len(norms), f"{label}: {len(kn)} norm taps in the oracle, {len(norms)} norm launches in the engine"
    assert [kind(k) for k in kb] == [b[0] for b in buffers], \
        f"{label}: tape order differs from oracle call order: {[kind(k) for k in kb]} vs {[b[0] for b in buffers]}"
    worst, where = {}, {}
    for key, got in list(zip(kn, norms)) + list(zip(kb, (b[1] for b in buffers))):
        ref = _as_rows(taps[key], got)
        assert ref.numel() == got.numel() and ref.shape[-1] == got.shape[-1], \
            f"{label}: {key}: oracle {tuple(taps[key].shape)} vs engine buffer {tuple(got.shape)}"
        e = rel(got.float(), ref.to(got.device).reshape(got.shape))
        kd = kind(key)
        if not e <= worst.get(kd, -1.0):  # (a NaN replaces anything)
            worst[kd], where[kd] = e, key
    for kd in sorted(worst):
        print(f"[{label}] tap kind {kd:9s} worst rel {worst[kd]:.3e} (bar {TAP[family][kd]:.0e}) at {where[kd]}")
    bad = {kd: (e, where[kd]) for kd, e in worst.items() if not (math.isfinite(e) and e < TAP[family][kd])}
    assert not bad, f"{label}: taps beyond their bars: {bad}"
    return worst
