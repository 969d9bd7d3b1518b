"""Batched novel-view evaluation on the GPU: the per-sample object mapper (vneti_mapper_fwd_slots and its legacy input
layer), B different prompts in one sampler graph against B = 1 generations, the sub-batched VAE decode, and the
output-extent guards of the buffer-store launchers."""
import pytest
import torch

from helpers.checks import frob_rel as _rel

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bucket(states, n_each):
    """flat mappers at a 4-float aligned stride (the 16-byte load condition of every slot)"""
    from view_neti_amd.engine.text import flatten_mapper_state
    stride = (n_each + 3) // 4 * 4
    flat = torch.zeros(stride * len(states))
    for i, sd in enumerate(states):
        f = flatten_mapper_state(sd)
        assert f.numel() == n_each
        flat[i * stride:i * stride + n_each] = f
    return flat.to(DEV), stride


def _mapper_states(n, E, h, D, seed, legacy_pe=None):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc_=0.1: torch.randn(*s, generator=gen) * sc_
    out = []
    for _ in range(n):
        sd = {"net.0.weight": rn(h, E, sc_=0.15), "net.0.bias": rn(h), "net.1.weight": 1 + rn(h), "net.1.bias": rn(h),
              "net.3.weight": rn(h, h), "net.3.bias": rn(h), "net.4.weight": 1 + rn(h), "net.4.bias": rn(h),
              "output_layer.0.weight": rn(2 * D, h, sc_=0.15), "output_layer.0.bias": rn(2 * D)}
        if legacy_pe is not None:
            sd["input_layer.weight"] = rn(E, 2 * legacy_pe.shape[0], sc_=0.02)
            sd["input_layer.bias"] = rn(E)
        out.append(sd)
    return out


@pytest.mark.parametrize("legacy", [False, True])
def test_mapper_fwd_slots_matches_single_slot_launches(legacy):
    """slots [2, 0, 1, 2] over a 3-mapper bucket: every row r = l*Bn + b bit-equal to mapper_fwd run with slot slots[b]"""
    from view_neti_amd import ops
    from view_neti_amd.mapper import fourier_frequencies
    nl, Bn, D = 16, 4, 64
    E, h = (160, 128) if legacy else (64, 64)
    slots_h = [2, 0, 1, 2]
    t = torch.tensor([17, 803, 400, 999], device=DEV)
    w_pe = (torch.randn(1024, 2, generator=torch.Generator().manual_seed(3)) * torch.tensor([0.03, 2.0])).to(DEV) \
        if legacy else None
    states = _mapper_states(3, E, h, D, 11, w_pe)
    n_std = ops.mapper_num_params(E, h, D, True)
    n_each = n_std + (ops.mapper_legacy_input_params(E, 2048) if legacy else 0)
    bucket, stride = _bucket(states, n_each)
    R = nl * Bn
    w_enc = fourier_frequencies([0.03, 2.0], E, 0).to(DEV)
    data = torch.empty(R, 2, device=DEV)
    ops.mapper_inputs(t, None, data, nl, Bn)
    slots = torch.tensor(slots_h, dtype=torch.int32, device=DEV)

    def run(per_sample, s):
        word = torch.full((R, D), float("nan"), device=DEV)
        byp = torch.full((R, D), float("nan"), device=DEV)
        save = torch.zeros(ops.mapper_save_floats(R, E, h), device=DEV)
        enc = None
        if legacy:
            enc = torch.full((R, E), float("nan"), device=DEV)
            if per_sample:
                ops.mapper_legacy_input_fwd_slots(bucket[n_std:], slots, stride, t, w_pe, enc, nl, Bn, E, 2048)
            else:
                ops.mapper_legacy_input_fwd(bucket[n_std:], t, w_pe, enc, nl, Bn, E, 2048, s, stride)
        d, we = (None, None) if legacy else (data, w_enc)
        if per_sample:
            ops.mapper_fwd_slots(bucket, slots, stride, Bn, d, we, None, 0.4, word, byp, save, R, E, h, D, True, enc_in=enc)
        else:
            ops.mapper_fwd(bucket, d, we, None, 0.4, word, byp, save, R, E, h, D, True, s, stride, enc_in=enc)
        return word.cpu(), byp.cpu(), save.view(R, -1).cpu(), (enc.cpu() if legacy else None)

    got = run(True, None)
    for s in range(3):
        ref = run(False, torch.tensor([s], dtype=torch.int32, device=DEV))
        rows = [l * Bn + b for l in range(nl) for b in range(Bn) if slots_h[b] == s]
        for g, r in zip(got, ref):
            if g is not None:
                assert torch.equal(g[rows], r[rows]), f"slot {s}: per-sample rows differ from the single-slot launch"
    assert all(torch.isfinite(x).all() for x in got if x is not None)
    # the per-sample launch is not a single-slot launch in disguise: the three mappers give different words
    assert not torch.equal(got[0][0], got[0][1])


def _engine_setup(cfg_name, B, per_sample):
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine.infer import InferenceEngine
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    cfg = sc.CONFIGS[cfg_name]()
    D = cfg.clip.hidden_size
    gen = torch.Generator().manual_seed(9)
    mk = lambda: {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in init_mapper_state(64, 64, D).items()}
    with torch.random.fork_rng(devices=[]):  # init_mapper_state draws from the global RNG: same mappers on every call
        torch.manual_seed(9)
        objs, sdv = [mk(), mk()], mk()
    from view_neti_amd import ops
    bucket, stride = _bucket(objs, ops.mapper_num_params(64, 64, D, True))
    w_enc = fourier_frequencies([0.03, 2.0], 64, 0)
    w_enc_v = fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
    uw, dw, cw = synth.unet_weights(cfg.unet), synth.vae_decoder_weights(cfg.vae), synth.clip_weights(cfg.clip)
    slot = None if per_sample else torch.zeros(1, dtype=torch.int32, device=DEV)
    eng = InferenceEngine(cfg, uw, dw, cw, B, 64, 64, None, w_enc, 0.4, 0.2, mapper_view=sdv, w_enc_view=w_enc_v,
                          norm_scale_view=0.35, alpha_view=0.3, params_object=bucket, object_slot=slot,
                          object_slot_stride=stride, per_sample_slots=per_sample)
    return cfg, eng, slot


@pytest.mark.parametrize("cfg_name,kind,steps", [("tiny", "dpm++2m", 3), ("tiny21", "ddim", 3)])
def test_batched_prompts_match_single_prompt_generations(cfg_name, kind, steps):
    """B = 4 prompts (four view tokens, two objects, four seeds) in one sampler graph vs four B = 1 generations"""
    from view_neti_amd import synth
    gs, B = 5.0, 4
    cfg, eng, _ = _engine_setup(cfg_name, B, True)
    V = cfg.clip.vocab_size
    obj_ids, view_ids = [V - 3, V - 5], [V - 4, V - 6, V - 7, V - 8]
    objs = [0, 1, 1, 0]
    rows = []
    for b in range(B):
        r = synth.input_ids(1, obj_ids[objs[b]], V, view_placeholder_id=view_ids[b])
        rows.append(torch.roll(r, b, dims=1) if b % 2 else r)
    ids = torch.cat(rows)
    vparams = synth.gaussian((B, 12), 9).clamp(-1, 1)
    neg = synth.input_ids(1, obj_ids[0], V)
    neg[neg == obj_ids[0]] = 7
    seeds = [3, 1, 4, 1]
    lat = torch.cat([torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(s)) for s in seeds])
    eng.set_negative_prompt(neg)
    po = torch.tensor([obj_ids[o] for o in objs])
    eng.set_prompts(ids, po, torch.tensor(view_ids), vparams, slots=objs)
    img = eng.generate(lat, steps, gs, kind).cpu().clone()
    x = eng.x.cpu().clone()
    img_eager = eng.generate(lat, steps, gs, kind, use_graph=False).cpu()
    assert torch.equal(eng.x.cpu(), x) and torch.equal(img_eager, img), "graph replay must match the eager loop bit for bit"
    with pytest.raises(ValueError):
        eng.set_prompts(ids, torch.tensor([obj_ids[0], -1, -1, -1]), torch.tensor(view_ids), vparams, slots=objs)
    with pytest.raises(ValueError):
        eng.set_prompts(ids, po, torch.tensor(view_ids), vparams, slots=objs, truncation_idx=[None, 3, None, None])
    with pytest.raises(ValueError):
        eng.set_prompts(ids, po, torch.tensor(view_ids), vparams, slots=[0, 1, 2, 0])
    del eng
    _, one, slot = _engine_setup(cfg_name, 1, False)
    one.set_negative_prompt(neg)
    worst_img, worst_x = 0.0, 0.0
    for b in range(B):
        slot.fill_(objs[b])
        one.set_prompt(ids[b:b + 1], po[b:b + 1], torch.tensor(view_ids[b:b + 1]), vparams[b:b + 1])
        ib = one.generate(lat[b:b + 1], steps, gs, kind).cpu()
        ei = (img[b] - ib[0]).abs().mean().item()
        ex = _rel(x[b], one.x[0])
        worst_img, worst_x = max(worst_img, ei), max(worst_x, ex)
    print(f"[batched prompts {cfg_name} {kind} B={B}] vs B=1: image mean abs err max {worst_img:.3e}; "
          f"final latents rel max {worst_x:.3e}")
    assert worst_img < 1e-2 and worst_x < 2e-2


def test_sub_batched_decode_matches_whole_batch(monkeypatch):
    from view_neti_amd import sd_config as sc, synth
    from view_neti_amd.engine import infer
    from view_neti_amd.engine.vae import VAEDecoderEngine
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    cfg = sc.tiny()
    B = 4
    monkeypatch.setattr(infer, "decode_sub_batch", lambda vae, h, w, batch: 2)
    dw, cw = synth.vae_decoder_weights(cfg.vae), synth.clip_weights(cfg.clip)
    eng = infer.InferenceEngine(cfg, synth.unet_weights(cfg.unet), dw, cw, B, 64, 64,
                                init_mapper_state(64, 64, cfg.clip.hidden_size), fourier_frequencies([0.03, 2.0], 64, 0),
                                0.4)
    assert eng.decoder.B == 2 and eng.image.shape == (B, 64, 64, 3)
    z = synth.gaussian((B, 4, 8, 8), 21)
    eng.x.copy_(z)
    sub = eng.decode().cpu()
    whole = VAEDecoderEngine(cfg.vae, dw, B, 8, 8)
    whole.z_in.copy_(z)
    whole.forward()
    ref = whole.image.cpu()
    err = (sub - ref).abs().max().item()
    print(f"[sub-batched decode] 2 x 2 vs 4: max abs {err:.3e}")
    assert err < 2e-3


def _strided_out(big, rows, cols, ld):
    assert (rows - 1) * ld + cols <= big.numel()
    return big.as_strided((rows, cols), (ld, 1))


def test_output_extent_guards_refuse_over_2gib():
    """each family of buffer-store launchers refuses an output whose addressed extent reaches 2 GiB, with the size in
    the message; the strided output views lie inside one real allocation just over 2 GiB, so no launch could address
    memory it does not own"""
    from view_neti_amd import ops, packing
    rows = 64
    ld = ((1 << 31) // (2 * (rows - 1)) + 64) // 8 * 8  # ((rows - 1) * ld + cols) * 2 bytes > 2 GiB
    big = torch.empty(rows * ld, dtype=torch.float16, device=DEV)
    assert big.numel() * 2 > (1 << 31)
    x16 = torch.randn(rows, 128, device=DEV).half()
    gamma, beta = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    mean, rstd = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)

    def refused(fn):
        with pytest.raises(RuntimeError) as e:
            fn()
        msg = str(e.value)
        assert "bytes" in msg and "2 GiB" in msg, msg
        return msg

    out = _strided_out(big, rows, 128, ld)
    refused(lambda: ops.add(x16, x16, out))
    refused(lambda: ops.sum2x2(torch.randn(4 * rows, 128, device=DEV).half(), out, 1, 8, 8, 128))
    refused(lambda: ops.layernorm_fwd(x16, out, gamma, beta, mean, rstd, 1e-5))
    ws = torch.zeros(ops.groupnorm_ws_floats(1, rows, 128, 32), device=DEV)
    refused(lambda: ops.groupnorm_fwd(x16, out, gamma, beta, torch.zeros(32, device=DEV), torch.zeros(32, device=DEV),
                                      ws, 1, rows, 128, 32, 1e-6, False))
    w_in = packing.conv_in_direct(torch.randn(128, 3, 3, 3)).half().to(DEV)
    img = torch.randn(1, 3, 8, 8, device=DEV)
    refused(lambda: ops.conv3x3_in(img, w_in, torch.zeros(128, device=DEV), out, 1, 3, 8, 8, img.stride()))
    wt = torch.randn(128, 128, device=DEV).half()
    msg = refused(lambda: ops.gemm(x16, wt, out))
    assert str(((rows - 1) * ld + 128) * 2) in msg
    torch.cuda.synchronize()
    # the same launches with an ordinary output still run
    ops.add(x16, x16, torch.empty(rows, 128, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()


def test_reference_inference_cli_end_to_end(tmp_path, monkeypatch):
    """train 2 steps on a DTU-shaped scene (mode 2), then the reference's evaluation command in a child process: all 34
    evaluation views x 2 seeds at 768 x 576, batched; PNGs and results_all_*.pt with the metric means; the batched
    images match B = 1 generations"""
    import os
    import subprocess
    import sys
    from pathlib import Path

    import numpy as np
    from PIL import Image
    from view_neti_amd.compat import config as C
    from view_neti_amd.compat import inference_dtu as nvs
    from view_neti_amd.compat.coach import Coach
    from view_neti_amd.compat.dataset import TextualInversionDataset
    monkeypatch.chdir(tmp_path)
    cal = tmp_path / "data" / "dtu" / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    rng = np.random.RandomState(1)
    mats = rng.randn(49, 3, 4) * np.array([[1e3, 1e3, 1e3, 1e5]])
    for i in range(49):
        np.savetxt(cal / f"pos_{i + 1:03d}.txt", mats[i])
    scan = tmp_path / "data" / "dtu" / "Rectified" / "scan114"
    scan.mkdir(parents=True)
    for c in range(49):
        Image.fromarray(rng.randint(0, 255, (120, 160, 3), dtype=np.uint8)).save(
            scan / TextualInversionDataset.dtu_cam_and_lighting_to_fname(c, "3"))
    cfg = C.parse(C.RunConfig, [
        "--learnable_mode", "2", "--data.train_data_dir", str(scan), "--data.placeholder_object_token", "<object>",
        "--data.camera_representation", "dtu-12d", "--data.dtu_subset", "3", "--data.dtu_preprocess_key", "1",
        "--data.augmentation_key", "5", "--data.dataloader_num_workers", "0", "--model.word_embedding_dim", "128",
        "--model.arch_view_net", "15", "--model.arch_view_disable_tl", "False", "--model.arch_mlp_hidden_dims", "64",
        "--model.use_nested_dropout", "False", "--model.pe_sigma_exp_key", "2", "--optim.max_train_steps", "2",
        "--optim.train_batch_size", "1", "--optim.gradient_accumulation_steps", "1", "--optim.mixed_precision", "fp16",
        "--log.save_steps", "2", "--eval.validation_steps", "1000", "--eval.num_denoising_steps", "2",
        "--log.exp_dir", str(tmp_path / "out"), "--log.exp_name", "m2"])
    cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
    cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
    torch.manual_seed(cfg.seed)
    Coach(cfg).train()
    run = cfg.log.exp_dir
    assert (run / "mapper-steps-2_view.pt").exists() and (run / "mapper-steps-2_object.pt").exists()
    root = Path(__file__).resolve().parents[1]
    yaml_path = tmp_path / "inference.yaml"
    yaml_path.write_text("input_dir: results/exp\niteration: 1500\nseeds: [0,1]\ntorch_dtype: fp16\n"
                         "num_denoising_steps: 30\n")
    cmd = ["timeout", "-k", "10", "300", sys.executable, str(root / "scripts" / "inference.py"), "--config_path",
           str(yaml_path), "--input_dir", str(run), "--iteration", "2", "--seeds", "[0,1]", "--num_denoising_steps", "2",
           "--batch", "4"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = run / "inference"
    for s in (0, 1):
        assert (out / nvs.preds_png_name(None, 2, s)).exists()
    res = torch.load(out / nvs.results_name(2, [None], [0, 1]), weights_only=False)
    assert list(res) == [None]
    means = {k: v for k, v in res[None].items() if k.endswith("_mean")}
    assert {"mse_train_mean", "mse_test_mean", "psnr_train_mean", "psnr_test_mean", "ssim_train_mean",
            "ssim_test_mean"} <= set(means) and all(np.isfinite(v) for v in means.values())
    assert len(res[None]["imgs_pred"]) == 2 and len(res[None]["imgs_pred"][0]) == 34
    # batched vs B = 1 on a few views (the same (object, camera, seed) triples; padding of a partial batch included)
    train_cfg = nvs.load_train_cfg(run, 2)
    train_cfg.log.exp_dir = run
    cams, seeds = [22, 25, 28], [0, 1]
    got = {}
    for b in (4, 1):
        pipe, pm = nvs.load_nvs_pipeline(train_cfg, 2, b)
        assert (pipe.engine.h * 8, pipe.engine.w * 8) == (576, 768)
        got[b] = nvs.generate_views(pipe, pm, pipe.object_tokens, cams, seeds, 2)[pipe.object_tokens[0]]
        del pipe, pm
    worst = max(np.abs(got[4][c].astype(np.float64) - got[1][c]).mean() / 255 for c in cams)
    print(f"[nvs cli] batch 4 vs batch 1: image mean abs err max {worst:.3e}; metric means {means}")
    assert worst < 1e-2
