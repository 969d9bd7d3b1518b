"""Held-out validation on the GPU: the per-sample MSE kernel against float64 torch (fp16 here, the bf16
library in a child process), `TrainStepEngine.eval_losses` against the CPU oracle and for the absence of side effects, and
the Coach end to end on a synthetic DTU scene — heldout-loss.jsonl, the offline CLI, and the opt-in 34-view validation."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from helpers.bf16_child import run_bf16_child
from helpers.checks import DEV
from helpers.coach_runs import dtu_scene as _dtu_scene, mode2_cfg as _mode2_cfg, train_from_cfg as _train
from helpers.engines import INIT_ALL_FIRST, STATE_PLUS as _STATE_PLUS, batch_dict as _batch, build_train_engine
from helpers.engines import feed_dict as _set, snapshot

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# ================================================================================================ kernel
# the pixel chunk one block of vneti_mse_loss_per_sample reduces (csrc/elementwise.hip kMseChunk): a sample of HW pixels is
# cdiv(HW, 256) blocks, whatever the batch
CHUNK = 256
SHAPES = ([(1, 4, 4, 1)] + [(hw, 4, ldp, 3) for hw in (63, 64, 65) for ldp in (4, 8, 320)]
          + [(hw, 4, 4, 3) for hw in (CHUNK - 1, CHUNK, CHUNK + 1)] + [(4096, 4, 4, 3)])
# ten times the pairwise-summation bound log2(n) 2^-24 at n = 16384; the inputs are rounded to the 16-bit format first, so
# the float64 reference sees the values the kernel sees
REL_TOL = 1e-5


def _inputs(HW, Lc, ldp, B, seed=0):
    from view_neti_amd import lib
    g = torch.Generator().manual_seed(1000 * HW + ldp + seed)
    wide = torch.randn((B * HW, ldp), generator=g).to(lib.act_dtype())
    target = torch.randn((B, Lc, HW), generator=g)
    return wide, target


def _ref64(wide, target, B, Lc, HW):
    p = wide[:, :Lc].double().view(B, HW, Lc).permute(0, 2, 1)
    return ((p - target.double()) ** 2).mean(dim=(1, 2))


def _run(wide, target, B, Lc, HW):
    from view_neti_amd import ops
    wd, td = wide.to(DEV), target.to(DEV).contiguous()
    out = torch.full((B,), -1.0, device=DEV)
    ws = torch.zeros(ops.mse_loss_per_sample_ws_floats(B, HW), device=DEV)
    ops.mse_loss_per_sample(wd[:, :Lc], td, out, ws, B, Lc, HW)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("HW,Lc,ldp,B", SHAPES)
def test_mse_per_sample_matches_float64(HW, Lc, ldp, B):
    from view_neti_amd import ops
    wide, target = _inputs(HW, Lc, ldp, B)
    ref = _ref64(wide, target, B, Lc, HW)
    got = _run(wide, target, B, Lc, HW)
    rel = ((got.double() - ref).abs() / ref).max().item()
    print(f"[mse_per_sample HW={HW} Lc={Lc} ldp={ldp} B={B}] max rel err {rel:.2e}")
    assert rel <= REL_TOL
    assert torch.equal(got, _run(wide, target, B, Lc, HW)), "two calls must be bit-equal"
    # the same numbers as the training loss: sum(out) Lc HW against vneti_mse_loss_grad's loss_sum on the same inputs
    wd, td = wide.to(DEV), target.to(DEV).contiguous()
    dp = torch.zeros_like(wd)
    loss_sum = torch.zeros(1, device=DEV)
    ops.mse_loss_grad(wd[:, :Lc], td, dp[:, :Lc], loss_sum, torch.ones(3, device=DEV), B, Lc, HW)
    total, want = got.double().sum().item() * Lc * HW, float(loss_sum.item())
    print(f"[mse_per_sample HW={HW} ldp={ldp}] sum(out) Lc HW {total:.8e} vs loss_sum {want:.8e} rel {abs(total - want) / want:.2e}")
    assert abs(total - want) / want <= 1e-6


@pytest.mark.parametrize("HW", [65, CHUNK + 1, 4096])
def test_mse_per_sample_value_is_independent_of_batch_and_position(HW):
    Lc, ldp = 4, 8
    wide, target = _inputs(HW, Lc, ldp, 3)
    base = _run(wide, target, 3, Lc, HW)
    rows, tg = wide[HW:2 * HW], target[1:2]  # sample 1 of 3 ...
    alone = _run(rows, tg, 1, Lc, HW)  # ... as the only sample
    fw, ft = _inputs(HW, Lc, ldp, 5, seed=7)
    fw[4 * HW:] = rows
    ft[4] = tg[0]
    last = _run(fw, ft, 5, Lc, HW)  # ... and as sample 4 of 5
    assert torch.equal(alone[0], base[1]) and torch.equal(last[4], base[1])


def test_mse_per_sample_non_finite_stays_in_its_sample():
    HW, Lc, ldp, B = CHUNK + 1, 4, 8, 3
    wide, target = _inputs(HW, Lc, ldp, B)
    clean = _run(wide, target, B, Lc, HW)
    for bad, where in ((float("nan"), HW + 3), (float("inf"), 2 * HW - 1)):  # first and last chunk of sample 1
        w2 = wide.clone()
        w2[where, 2] = bad
        got = _run(w2, target, B, Lc, HW)
        assert not math.isfinite(got[1].item())
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]) and math.isfinite(got[0].item())
    w2 = wide.clone()
    w2[HW, Lc] = float("nan")  # a padding column of a wider row is not read
    assert torch.equal(_run(w2, target, B, Lc, HW), clean)


def test_mse_per_sample_refuses_bad_arguments():
    from view_neti_amd import lib, ops
    L = lib.load()
    HW, Lc, B = 64, 4, 2
    wide, target = _inputs(HW, Lc, 8, B)
    wd, td = wide.to(DEV), target.to(DEV)
    out, ws = torch.zeros(B, device=DEV), torch.zeros(ops.mse_loss_per_sample_ws_floats(B, HW), device=DEV)
    st = ops.stream()
    good = (wd.data_ptr(), 8, td.data_ptr(), out.data_ptr(), ws.data_ptr(), B, Lc, HW, st)
    assert L.vneti_mse_loss_per_sample(*good) == 0
    EARG = -1
    for i, v in ((0, None), (2, None), (3, None), (4, None), (5, 0), (5, 65536), (6, 0), (7, 0), (1, Lc - 1)):
        args = list(good)
        args[i] = v
        assert L.vneti_mse_loss_per_sample(*args) == EARG, f"argument {i} = {v}"
        assert "mse_loss_per_sample" in lib.last_error()
    torch.cuda.synchronize()
    assert lib.query("mse_loss_per_sample_ws_floats", 0, HW) < 0 and lib.query("mse_loss_per_sample_ws_floats", B, 0) < 0
    assert ops.mse_loss_per_sample_ws_floats(3, CHUNK + 1) == 3 * 2 and ops.mse_loss_per_sample_ws_floats(3, CHUNK) == 3


def test_mse_per_sample_bf16_library(tmp_path):
    """a process computes in one 16-bit format: the kernel cases above again in a child with the -DVN_BF16 build"""
    from view_neti_amd import lib
    if lib.precision() == "bf16":
        return  # the whole file run under VNETI_PRECISION=bf16: the cases above already were the bf16 run
    run_bf16_child(str(Path("tests") / "test_heldout_gpu.py"), "mse_per_sample and not bf16_library", 120, tmp_path,
                   least=len(SHAPES) + 5, expect=len(SHAPES) + 3 + 1 + 1)


# ================================================================================================ engine
def _build(cfg_name, B, H=64, W=64, **kw):
    """object + view mapper on the tiny shape families, the global generator left as it was found"""
    kw.setdefault("lr", 1e-3)
    return build_train_engine(cfg_name, B, H, W, with_view=True, fork_rng=True, order=INIT_ALL_FIRST, **kw)


def _eval(eng, b, graph=True):
    _set(eng, b, for_eval=True)
    eng.set_noise(b["eps"], b["noise"], b["t"])
    return eng.eval_losses(graph=graph)


def _snapshot(eng):
    assert set(eng._STATE) <= set(_STATE_PLUS)
    return snapshot(eng, _STATE_PLUS)


@pytest.mark.parametrize("cfg_name", ["tiny", "tiny21"])
def test_eval_losses_match_oracle_without_side_effects(cfg_name):
    """per-sample losses against the per-sample MSE of the oracle's prediction and target (the project's 1e-3 loss bar);
    eager == graph bit for bit; every state tensor, the gradients, loss_sum and the text mode untouched"""
    from oracle import sd_ref as R
    B = 3
    cfg, eng, (uw, vw, cw), sd, w_enc, extra = _build(cfg_name, B, device_rng=False)
    b, ev = _batch(cfg, B), _batch(cfg, B, seed=5)
    first = _eval(eng, ev, graph=False)  # with the mappers the oracle below is given
    _set(eng, b)
    eng.set_noise(b["eps"], b["noise"], b["t"])
    eng.step_eager()  # moments, gradients and a loss_sum that are not zero
    torch.cuda.synchronize()
    before, mode = _snapshot(eng), eng.text.training
    eager = _eval(eng, ev, graph=False)
    assert not torch.equal(eager, first), "the evaluation reads the live mappers"
    graph = _eval(eng, ev, graph=True)
    again = _eval(eng, ev, graph=True)
    assert eager.dtype == torch.float32 and eager.device.type == "cpu" and tuple(eager.shape) == (B,)
    assert torch.equal(eager, graph) and torch.equal(graph, again), "eager and graph replays must be bit-equal"
    assert eng.graph_eval is not None and eng.text.training is mode
    after = _snapshot(eng)
    for n in _STATE_PLUS:
        assert torch.equal(before[n], after[n]), f"eval_losses() changed {n}"
    r16 = lambda d: {k: (v.half().float() if v.dim() >= 2 and "embedding" not in k else v) for k, v in d.items()}
    view = dict(p=extra["mapper_view"], w_enc=extra["w_enc_view"], norm_scale=0.35, placeholder=ev["pv"], params=ev["vp"],
                alpha=0.3, unconstrained=False)
    with torch.no_grad():
        _, aux = R.train_step_loss(cfg, r16(uw), r16(vw), r16(cw), sd, w_enc, 0.4, ev["px"], ev["ids"], ev["po"], ev["t"],
                                   ev["eps"], ev["noise"], alpha=0.2, view=view)
        target = ev["noise"] if cfg.ddpm.prediction_type == "epsilon" else \
            R.get_velocity(R.alphas_cumprod(cfg.ddpm), aux["latents"], ev["noise"], ev["t"])
        ref = ((aux["pred"].float() - target.float()) ** 2).mean(dim=(1, 2, 3))
    rel = ((first - ref).abs() / ref).max().item()
    print(f"[eval_losses {cfg_name}] gpu {first.tolist()} oracle {ref.tolist()} max rel {rel:.2e}")
    assert rel < 1e-3
    # a forward-only engine (what the offline CLI builds) runs the same launches
    _, fo, _, _, _, _ = _build(cfg_name, B, device_rng=False, need_backward=False)
    fo.params.copy_(eng.params)
    assert torch.equal(_eval(fo, ev), graph)


def test_training_is_not_perturbed_by_evaluations():
    """four captured train steps with an evaluation (other images, other noise) after each == four steps without"""
    B = 3
    outs = []
    for with_eval in (False, True):
        cfg, eng, _, _, _, _ = _build("tiny", B, device_rng=True, seed=5)
        b, ev = _batch(cfg, B), _batch(cfg, B, seed=5)
        _set(eng, b)
        eng.capture()
        for _ in range(4):
            _set(eng, b)
            eng.step()
            if with_eval:
                assert torch.isfinite(_eval(eng, ev)).all()
        torch.cuda.synchronize()
        outs.append((eng.params.clone(), eng.exp_avg_sq.clone(), eng.rng_state.clone(), int(eng.opt_step.item())))
    assert outs[0][3] == outs[1][3] == 4
    for a, c in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, c)


def test_eval_losses_ignore_nested_dropout_and_recapture():
    B = 3
    res = []
    for prob in (0.5, 0.0):
        cfg, eng, _, _, _, _ = _build("tiny", B, device_rng=True, seed=5, nested_dropout_prob=prob)
        assert (eng.text.hidden_mask_obj is not None) == (prob > 0) and eng.text.training
        ev = _batch(cfg, B, seed=5)
        res.append((_eval(eng, ev, graph=False), _eval(eng, ev, graph=True)))
        if prob > 0:
            first = eng.graph_eval
            _set(eng, _batch(cfg, B))
            eng.capture()  # re-captures the evaluation graph with the others
            assert eng.graph_eval is not None and eng.graph_eval is not first
            assert torch.equal(_eval(eng, ev), res[-1][1]) and eng.text.training
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[0][1])


def test_eval_losses_leave_the_moment_cache_alone():
    """a cached step after an evaluation on other images is bit-identical to the same step without the evaluation"""
    B = 3
    outs = []
    for with_eval in (False, True):
        cfg, eng, _, _, _, _ = _build("tiny", B, device_rng=True, seed=5, moment_cache_images=4)
        b, ev = _batch(cfg, B), _batch(cfg, B, seed=5)
        _set(eng, b, image_idx=[0, 1, 2])
        eng.capture()
        eng.step()  # (the capture's warm-up ran the encoder and filled slots 0..2)
        assert eng._cached_images == {0, 1, 2}
        if with_eval:
            cache, runs = eng.mcache.clone(), [0]
            fwd = eng.vae.forward
            eng.vae.forward = lambda: (runs.__setitem__(0, runs[0] + 1), fwd())[1]
            assert torch.isfinite(_eval(eng, ev, graph=False)).all() and runs[0] == 1, "the evaluation runs the encoder"
            eng.vae.forward = fwd
            assert torch.isfinite(_eval(eng, ev)).all()
            assert eng._cached_images == {0, 1, 2} and torch.equal(eng.mcache, cache)
        _set(eng, b, image_idx=[0, 1, 2])
        assert eng._use_cache()
        eng.step()  # served from the cache
        torch.cuda.synchronize()
        # (not loss_sum: vneti_mse_loss_grad adds its block partials with float atomics, in whatever order they finish)
        outs.append((eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.grads.clone(), eng.rng_state.clone()))
    assert all(torch.equal(a, c) for a, c in zip(outs[0], outs[1]))


def test_eval_losses_inside_an_accumulation_group_raise():
    B = 3
    cfg, eng, _, _, _, _ = _build("tiny", B, device_rng=True, seed=5, grad_accum=2)
    b = _batch(cfg, B)
    _set(eng, b)
    assert eng.step() is False and eng.micro == 1
    with pytest.raises(ValueError, match="accumulation"):
        eng.eval_losses()
    assert eng.step() is True
    assert torch.isfinite(_eval(eng, b)).all()
    with pytest.raises(RuntimeError, match="for_eval"):  # an evaluation batch is not trained on
        eng.step()
    _set(eng, b)
    assert eng.step() is False


# ================================================================================================ Coach
def _close(a, b, rel):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        return all(_close(a[k], b[k], rel) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(x, y, rel) for x, y in zip(a, b))
    if isinstance(a, float):
        return abs(a - b) <= rel * abs(b)
    return a == b


def test_coach_heldout_loss_curve_and_offline_cli(tmp_path, monkeypatch):
    """mode 2, 4 steps, an evaluation every 2: records at steps 2 and 4 over the 34 cameras x K = 4 split as get_cam_idxs
    splits them; the mappers are bit-identical to the run without the evaluation (nested dropout and augmentations on: the
    torch, numpy, python and device generators all matter); the offline CLI reproduces the step-2 record"""
    from view_neti_amd.compat import heldout as H
    from view_neti_amd.compat.dtu_metrics import get_cam_idxs
    monkeypatch.chdir(tmp_path)
    (scan,) = _dtu_scene(tmp_path, ["scan114"])
    on = _train(_mode2_cfg(scan, tmp_path / "out", "on", "--eval.heldout_loss_steps", "2"))
    off = _train(_mode2_cfg(scan, tmp_path / "out", "off"))
    assert off.heldout is None and not (off.cfg.log.exp_dir / H.FILE_NAME).exists()
    assert torch.equal(on.engine.params, off.engine.params), "the evaluation must not perturb training"
    assert torch.equal(on.engine.rng_state, off.engine.rng_state)
    run = on.cfg.log.exp_dir
    recs = H.read_records(run / H.FILE_NAME)
    assert [r["step"] for r in recs] == [2, 4] and all(r["timesteps"] == [125, 375, 625, 875] for r in recs)
    cams, train, test = get_cam_idxs(3)
    plan = on.heldout.plan
    assert plan.cams == cams and plan.cams_train == train and plan.cams_test == test
    assert plan.n_items("<object>") == 34 * 4 and len(plan.batches["<object>"]) == 46
    scored = [it for it, _ in on.heldout.evaluate()["<object>"]]
    assert len(scored) == 34 * 4 and {it.cam for it in scored if it.split == "train"} == set(train)
    for r in recs:
        o = r["objects"]["<object>"]
        assert list(r["objects"]) == ["<object>"] and sorted(o["by_view"]) == cams
        vals = [o["train"], o["test"]] + list(o["by_view"].values()) + [v for t in o["by_timestep"].values() for v in t.values()]
        assert all(isinstance(v, float) and math.isfinite(v) and v > 0 for v in vals)
    assert recs[0]["objects"] != recs[1]["objects"], "the mappers moved between steps 2 and 4"
    assert "heldout loss step 2" in (run / "logs" / "log.txt").read_text()
    # the new keys stay out of the checkpoint's cfg
    ck = torch.load(run / "mapper-steps-2_view.pt", map_location="cpu", weights_only=False)
    assert "heldout_loss_steps" not in ck["cfg"]["eval"]
    assert "eval.heldout_loss_steps" not in ck.get("vneti_ext", {}).get("config_ext", {})
    # offline, in this process (same autotuner picks): bit-equal to what the run wrote at step 2
    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        import heldout_loss as cli
    finally:
        sys.path.pop(0)
    listing = {f.name: f.stat().st_mtime_ns for f in run.rglob("*") if f.is_file()}
    (rec,) = cli.main(["--input_dir", str(run), "--iterations", "[2]"])
    assert json.loads(json.dumps(rec)) == json.loads((run / H.FILE_NAME).read_text().splitlines()[0])
    assert H.read_records(run / H.OFFLINE_FILE_NAME)[0]["step"] == 2
    now = {f.name: f.stat().st_mtime_ns for f in run.rglob("*") if f.is_file()}
    assert {k: v for k, v in now.items() if k != H.OFFLINE_FILE_NAME} == listing, "the CLI writes its own file only"
    # and as the command a user runs, in a process of its own: to the project's 1e-3 loss bar
    (run / H.OFFLINE_FILE_NAME).unlink()
    cmd = ["timeout", "-k", "10", "240", sys.executable, str(ROOT / "scripts" / "heldout_loss.py"), "--input_dir", str(run),
           "--iterations", "[2]"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "iteration" in r.stdout and "train" in r.stdout and "test" in r.stdout
    (child,) = H.read_records(run / H.OFFLINE_FILE_NAME)
    assert _close(child, recs[0], 1e-3)


M3_YAML = """
learnable_mode: 3
log: {{exp_name: m3, exp_dir: {out}, save_steps: 100}}
data: {{train_data_dir: data/dtu/Rectified, train_data_subsets: [scan65, scan125], super_category_object_tokens: [object, object],
       placeholder_object_tokens: [<scan65>, <scan125>], placeholder_object_token: <object>, dataloader_num_workers: 0,
       camera_representation: dtu-12d, dtu_subset: 3, dtu_lighting: 3, dtu_preprocess_key: 1, augmentation_key: 0}}
model: {{arch_mlp_hidden_dims: 64, use_nested_dropout: False, word_embedding_dim: 128, arch_view_net: 15,
        arch_view_disable_tl: False, pe_sigma_exp_key: 2}}
eval: {{validation_steps: 1000, eval_placeholder_object_tokens: [<scan65>, <scan125>], heldout_loss_steps: 2,
       heldout_loss_timesteps: 2}}
optim: {{max_train_steps: 2, train_batch_size: 2, gradient_accumulation_steps: 1, mixed_precision: fp16}}
"""


def test_coach_heldout_mode3_one_entry_per_object(tmp_path, monkeypatch):
    from view_neti_amd.compat import config as C
    from view_neti_amd.compat import heldout as H
    monkeypatch.chdir(tmp_path)
    _dtu_scene(tmp_path, ["scan65", "scan125"])
    y = tmp_path / "m3.yaml"
    y.write_text(M3_YAML.format(out=str(tmp_path / "out")))
    cfg = C.parse(C.RunConfig, ["--config_path", str(y)])
    cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
    cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
    coach = _train(cfg)
    slots = []
    orig = coach.engine.set_batch
    coach.engine.set_batch = lambda *a, **k: (slots.append(k["object_index"]), orig(*a, **k))[1]
    rows = coach.heldout.evaluate()
    assert set(slots[:34]) == {0} and set(slots[34:]) == {1} and len(slots) == 68, "object_index follows the object"
    (rec,) = H.read_records(cfg.log.exp_dir / H.FILE_NAME)
    assert rec["step"] == 2 and rec["timesteps"] == [250, 750] and list(rec["objects"]) == ["<scan65>", "<scan125>"]
    for tok in ("<scan65>", "<scan125>"):
        assert len(rows[tok]) == 34 * 2 and all(math.isfinite(v) for _, v in rows[tok])
        for cam in (22, 0):
            assert coach.heldout.image_path[(tok, cam)].parent.name == tok[1:-1], "each object is scored on its own scene"
    a, b = (rec["objects"][t]["by_view"] for t in ("<scan65>", "<scan125>"))
    assert all(a[c] != b[c] for c in a)
    # a scene without its evaluation views stops the run at construction
    (tmp_path / "data" / "dtu" / "Rectified" / "scan125" / "rect_001_3_r5000.png").unlink()
    from view_neti_amd.compat.coach import Coach
    with pytest.raises(FileNotFoundError, match="camera 0"):
        Coach(cfg)


def test_coach_validation_nvs_renders_the_34_views(tmp_path, monkeypatch):
    """eval.validation_nvs: the reference's validation files — all 34 evaluation cameras at 768 x 576, the metric means —
    from the live mappers, equal to what the evaluation command renders from the checkpoint of the same step; and with the
    switch off, the files of a run are what they always were.  `inference_dtu.run` keeps no raw images (it writes figures
    and the 300 x 400 tensors of the metric harness), so the comparison is with the two calls it makes to render them,
    `load_nvs_pipeline` and `generate_views`, with its arguments: the uint8 images must be `np.array_equal`."""
    from view_neti_amd.compat import inference_dtu as nvs
    from view_neti_amd.compat.dtu_metrics import get_cam_idxs
    monkeypatch.chdir(tmp_path)
    (scan,) = _dtu_scene(tmp_path, ["scan114"])
    common = ("--optim.max_train_steps", "2", "--optim.train_batch_size", "1", "--eval.validation_steps", "2")
    on = _train(_mode2_cfg(scan, tmp_path / "out", "nvs", *common, "--eval.validation_nvs", "True"))
    run = on.cfg.log.exp_dir
    stem = "validation-iter_2-denoisesteps_2"
    val = torch.load(run / f"{stem}_numseeds_1_upsample_1.pt", weights_only=False)
    cams, _, _ = get_cam_idxs(3)
    assert sorted(val) == cams and len(cams) == 34
    assert all(v.shape == (1, 576, 768, 3) and v.dtype == np.uint8 for v in val.values())
    assert (run / f"{stem}_numseeds_1_upsample_1_seed_0.png").exists()
    metrics = json.loads((run / f"{stem}_metrics.json").read_text())
    assert list(metrics) == ["<object>"]
    assert set(metrics["<object>"]) == {f"{m}_{s}_mean" for m in ("mse", "psnr", "ssim", "lpips") for s in ("train", "test")}
    assert all(math.isfinite(v) for v in metrics["<object>"].values())
    assert on.validator.engine.text.mo.params.data_ptr() == on.engine.params.data_ptr(), "the live bucket, not a copy"
    assert on.validator.engine.B == 4 and on.validator.engine.slots is not None
    train_cfg = nvs.load_train_cfg(run, 2)
    train_cfg.log.exp_dir = run
    pipe, pm = nvs.load_nvs_pipeline(train_cfg, 2, 4)
    ref = nvs.generate_views(pipe, pm, pipe.object_tokens, cams, [0], 2)["<object>"]
    assert all(np.array_equal(val[c], ref[c]) for c in cams)
    del pipe, pm
    # ---- switch off: training views only, at the training size, no metrics file
    off = _train(_mode2_cfg(scan, tmp_path / "out", "plain", *common))
    plain = off.cfg.log.exp_dir
    old = torch.load(plain / f"{stem}_numseeds_1_upsample_1.pt", weights_only=False)
    ds = off.train_dataset
    assert sorted(old) == sorted(ds.lookup_view_token_to_camidx[t] for t in ds.placeholder_view_tokens) and len(old) == 3
    assert all(len(v) == 1 and v[0].shape == (384, 512, 3) and v[0].dtype == np.uint8 for v in old.values())
    assert Image.open(plain / f"{stem}_numseeds_1_upsample_1_seed_0.png").size == (3 * 512, 384)
    assert not (plain / f"{stem}_metrics.json").exists()
    assert sorted(p.name for p in plain.glob("validation-iter_*")) == [f"{stem}_numseeds_1_upsample_1.pt",
                                                                       f"{stem}_numseeds_1_upsample_1_seed_0.png"]
    # a scene without its ground truth stops the run at construction, not at the first validation step
    from view_neti_amd.compat.coach import Coach
    (scan / "rect_002_3_r5000.png").unlink()
    with pytest.raises(FileNotFoundError, match=r"cameras \[1\]"):
        Coach(_mode2_cfg(scan, tmp_path / "out", "gone", *common, "--eval.validation_nvs", "True"))
