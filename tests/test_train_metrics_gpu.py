"""The per-step training record and gradient-norm clipping in `TrainStepEngine` and `Coach`, on
the tiny SD shape family at batch 2.

Bit equality (torch.equal) wherever the feature must not change the training: the record alone, and clipping with a bound
nothing reaches.  Parity with torch (float64 AdamW + clip_grad_norm_, float64 losses and norms) at `check32`'s bar / the
1e-5 relative bar of the held-out loss (f6) where it computes something new."""
import json
import math

import numpy as np
import pytest
import torch

from helpers import coach_runs as rt  # toys, mode0_cfg, coach, train_counting, end_state, assert_end
from helpers.checks import check32
from helpers.engines import FORMS, STATE, build_device_rng_engine as _build, feed_six as _feed, run_steps
from helpers.engines import six_steps as _six_steps  # (the cache of its runs is shared with tests/test_loss_options_gpu.py)

pytestmark = pytest.mark.gpu

B, H, W, LR = 2, 64, 64, 3e-3
ROWS = 16


def _steps(cfg, eng, steps, mode3):
    run_steps(cfg, eng, steps, mode3, _feed)


@pytest.mark.parametrize("form", list(FORMS))
def test_record_leaves_the_training_bit_identical(form):
    plain, _, _ = _six_steps(form)
    rec, (rows, lost), _ = _six_steps(form, telemetry_rows=ROWS)
    for f in STATE:
        assert torch.equal(plain[f], rec[f]), f"{form}: {f} differs with the record on"
    accum = FORMS[form][1]
    assert lost == 0 and len(rows) == 6 * accum and [r["micro_step"] for r in rows] == list(range(6 * accum))
    assert [r["micro"] for r in rows] == [m for _ in range(6) for m in range(accum)]
    assert [r["closed"] for r in rows] == [m == accum - 1 for _ in range(6) for m in range(accum)]
    closed = [r for r in rows if r["closed"]]
    assert all(r["clip_coef"] == 1.0 and not r["skipped"] and r["lr"] == float(np.float32(LR)) for r in closed)
    assert all(0 < r["grad_norm"]["total"] < math.inf for r in closed)
    # growth_interval 3: the scale of steps 1-3, doubled for steps 4-6
    assert [r["loss_scale"] for r in closed] == [65536.0] * 3 + [131072.0] * 3
    if FORMS[form][0]:
        assert all(set(r["grad_norm"]) == {"total", "object", "view"} for r in closed)
        assert all(r["grad_norm"]["total"] == pytest.approx(math.hypot(r["grad_norm"]["object"], r["grad_norm"]["view"]),
                                                            rel=1e-6) for r in closed)
    else:
        assert all(set(r["grad_norm"]) == {"total", "object"} for r in closed)  # no view mapper in the bucket


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_unreachable_bound_is_the_unclipped_training(form):
    plain, _, _ = _six_steps(form)
    clipped, _, _ = _six_steps(form, max_grad_norm=1e30)
    for f in STATE:
        assert torch.equal(plain[f], clipped[f]), f"{form}: {f} differs with max_grad_norm=1e30"


# kernel launches behind each ABI call the feature adds (csrc/elementwise.hip); the _clipped AdamW entries launch what the
# unclipped ones launch
ADDED = {"mse_loss_per_sample": 2, "train_record": 1, "grad_sumsq": 1, "grad_norm_finish": 1}


@pytest.mark.parametrize("form", ["one-mapper", "mode3"])
def test_launch_budget(form, monkeypatch):
    """an eager step's ABI calls: with both off none of the new entries; with clipping at most 3 launches more, with the
    record and clipping at most 7 (grad_accum 1); everything else is the plain step's call list, in its order"""
    from view_neti_amd import lib
    mode3 = FORMS[form][0]

    def calls(**kw):
        cfg, eng = _build(mode3, 1, **kw)
        _feed(cfg, eng, 0, 0, mode3)
        names, orig = [], lib.call
        with monkeypatch.context() as m:
            m.setattr(lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
            assert eng.step()
        torch.cuda.synchronize()
        return names

    plain = calls()
    assert not [n for n in plain if n in ADDED or n.endswith("_clipped")] and "adamw_" in " ".join(plain)
    for kw, budget in ((dict(max_grad_norm=1.0), 3), (dict(telemetry_rows=ROWS), 7),
                       (dict(max_grad_norm=1.0, telemetry_rows=ROWS), 7)):
        got = calls(**kw)
        added = sum(ADDED.get(n, 0) for n in got)
        print(f"[launch budget {form} {sorted(kw)}] {added} launches added")
        assert 0 < added <= budget
        rest = [n[:-len("_clipped")] if n.endswith("_clipped") else n for n in got if n not in ADDED]
        assert rest == plain
        assert any(n.endswith("_clipped") for n in got) == ("max_grad_norm" in kw)


def _torch_losses(eng):
    Lc, hw = eng.cfg.vae.latent_channels, eng.h * eng.w
    pred = eng.unet.pred.double().view(B, hw, Lc).cpu()
    tgt = eng.target.double().view(B, Lc, hw).permute(0, 2, 1).cpu()
    return ((pred - tgt) ** 2).mean(dim=(1, 2))


def test_record_cross_check_overflow_and_recapture():
    """one eager engine with the record on: rows against torch, a forced overflow, and capture() after steps"""
    cfg, eng = _build(False, 1, telemetry_rows=ROWS)
    # ---- rows against float64 torch: losses from unet.pred / target, timesteps, the norm of the unscaled gradient
    for s in range(2):
        _feed(cfg, eng, s, 0, False)
        eng.forward_backward()
        torch.cuda.synchronize()
        want_loss, want_t = _torch_losses(eng), eng.timesteps.cpu().tolist()
        div = float(eng.scaler[0]) * float(eng.hyper[5])
        g = eng.grads.cpu()
        want64 = (torch.linalg.vector_norm(g.double()) / div).reshape(1)
        want32 = (torch.linalg.vector_norm(g) / div).reshape(1)
        eng.optimizer_step()
        rows, lost = eng.read_telemetry()
        assert lost == 0 and len(rows) == 1 and rows[0]["closed"] and rows[0]["micro_step"] == s
        row = rows[0]
        assert row["timesteps"] == want_t
        got = torch.tensor(row["losses"], dtype=torch.float64)
        err = ((got - want_loss).abs() / want_loss.abs()).max().item()
        print(f"[record step {s}] per-sample loss rel err {err:.3e}")
        assert err <= 1e-5
        check32(f"record step {s} grad_norm.total", torch.tensor([row["grad_norm"]["total"]]), want64, want32)
        assert row["loss_scale"] == div and not row["skipped"]
    assert eng.read_telemetry() == ([], 0)
    # ---- forced overflow (the approach of test_overflow_skips_step): a 2^40 loss scale overflows the f16 gradients
    eng.scaler[0] = 2.0 ** 40
    p0, step0 = eng.params.clone(), int(eng.opt_step)
    _feed(cfg, eng, 2, 0, False)
    assert eng.step()
    torch.cuda.synchronize()
    assert torch.equal(eng.params, p0) and int(eng.opt_step) == step0, "a skipped step must not touch the parameters"
    assert eng.step()
    rows, _ = eng.read_telemetry()
    assert [r["skipped"] for r in rows][0] is True and rows[0]["loss_scale"] == 2.0 ** 40 and rows[0]["clip_coef"] == 1.0
    assert rows[1]["loss_scale"] == 2.0 ** 39, "the halved scale appears on the next row"
    assert not math.isfinite(rows[0]["grad_norm"]["total"])
    # ---- capture() after steps: its warm-up steps leave no rows, the counter continues
    n = rows[-1]["micro_step"] + 1
    eng.scaler[0] = 65536.0
    eng.capture()
    assert eng.read_telemetry() == ([], 0)
    _steps(cfg, eng, (3, 4), False)
    rows, lost = eng.read_telemetry()
    assert lost == 0 and [r["micro_step"] for r in rows] == [n, n + 1] and all(r["closed"] for r in rows)
    # ---- more micro-steps than rows since the last read: the oldest are reported lost
    _steps(cfg, eng, range(5, 5 + ROWS + 3), False)
    rows, lost = eng.read_telemetry()
    assert lost == 3 and len(rows) == ROWS and [r["micro_step"] for r in rows] == list(range(n + 5, n + 5 + ROWS))


def test_clipping_against_torch():
    """max_grad_norm = half the first step's norm as the UNCLIPPED engine recorded it: the first update against float64
    torch AdamW + clip_grad_norm_ on the same gradient"""
    _, (rows, _), _ = _six_steps("one-mapper", telemetry_rows=ROWS)
    max_norm = 0.5 * rows[0]["grad_norm"]["total"]
    cfg, eng = _build(False, 1, telemetry_rows=ROWS, max_grad_norm=max_norm)
    assert eng.state_dict()["meta"]["max_grad_norm"] == max_norm
    _feed(cfg, eng, 0, 0, False)
    eng.forward_backward()
    torch.cuda.synchronize()
    p0, hyper = eng.params.cpu().clone(), eng.hyper.cpu().tolist()
    g = eng.grads.cpu() / (float(eng.scaler[0]) * hyper[5])
    eng.optimizer_step()
    (row,), _ = eng.read_telemetry()
    assert row["clip_coef"] < 1.0 and row["grad_norm"]["total"] == pytest.approx(rows[0]["grad_norm"]["total"], rel=1e-3)
    assert row["clip_coef"] == pytest.approx(0.5, rel=1e-2)
    refs = {}
    for dt in (torch.float64, torch.float32):
        q = p0.to(dt).clone().requires_grad_(True)
        opt = torch.optim.AdamW([q], lr=hyper[0], betas=(hyper[1], hyper[2]), eps=hyper[3], weight_decay=hyper[4])
        q.grad = g.to(dt)
        torch.nn.utils.clip_grad_norm_([q], max_norm)
        opt.step()
        refs[dt] = (q, opt)
    (q64, o64), (q32, o32) = refs[torch.float64], refs[torch.float32]
    check32("clipped first update p - p0", eng.params.cpu().double() - p0.double(), q64.detach() - p0.double(),
            q32.detach().double() - p0.double())
    check32("clipped first update m", eng.exp_avg, o64.state[q64]["exp_avg"], o32.state[q32]["exp_avg"])
    check32("clipped first update v", eng.exp_avg_sq, o64.state[q64]["exp_avg_sq"], o32.state[q32]["exp_avg_sq"])
    # the engine's own state refuses the other kind of run, naming the field; an old state (no such key) loads unclipped
    sd = eng.state_dict()
    _, plain = _build(False, 1)
    with pytest.raises(ValueError, match="max_grad_norm"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="max_grad_norm"):
        eng.load_state_dict(plain.state_dict())
    assert "max_grad_norm" not in plain.state_dict()["meta"]


# ------------------------------------------------------------------------------------------------ Coach
def _metrics(cfg):
    return (cfg.log.exp_dir / "train-metrics.jsonl").read_bytes()


@pytest.fixture(scope="module")
def toys(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("metrics")
    rt.toys(tmp / "toys")
    return tmp


def _run6(toys, name, extra):
    cfg = rt.mode0_cfg(toys / "toys", toys / name, "--log.train_metrics", "true", *extra)
    coach = rt.coach(cfg)
    assert rt.train_counting(coach) == 6
    return cfg, rt.end_state(coach), _metrics(cfg)


@pytest.fixture(scope="module")
def run_u(toys):
    """the uninterrupted, unclipped run of 6 steps (accumulation 2, batch 2, checkpoint + trainer state every 3)"""
    return _run6(toys, "ua", ())


def _check_lines(text, clipped):
    lines = [json.loads(l) for l in text.decode().splitlines()]
    assert [l["step"] for l in lines] == [1, 2, 3, 4, 5, 6]
    for l in lines:
        assert set(l) == {"step", "loss", "lr", "loss_scale", "skipped", "grad_norm", "clip_coef", "samples"}
        assert len(l["samples"]) == 2 * 2 and l["loss"] == pytest.approx(sum(s["loss"] for s in l["samples"]) / 4, rel=1e-12)
        assert set(l["grad_norm"]) == {"object", "total"} and all(0 <= s["t"] < 1000 for s in l["samples"])
        assert l["skipped"] is False and l["loss_scale"] == 65536.0
    assert len({l["lr"] for l in lines}) > 1, "the cosine schedule with warm-up moves the lr"
    assert lines[0]["clip_coef"] < 1.0 if clipped else all(l["clip_coef"] == 1.0 for l in lines)
    return lines


def _check_resume(toys, name, extra, cfg_a, end_a, text):
    """3 + 3: a run cut after step 3 and relaunched into the same directory continues the file byte for byte"""
    extra = ("--log.train_metrics", "true", *extra)
    cfg = rt.mode0_cfg(toys / "toys", toys / name, "--log.auto_resume", "true", *extra)
    coach = rt.coach(cfg)
    cfg.optim.max_train_steps = 3
    assert rt.train_counting(coach) == 3
    assert _metrics(cfg) == b"".join(l + b"\n" for l in text.splitlines()[:3])
    del coach
    with (cfg.log.exp_dir / "train-metrics.jsonl").open("a") as f:  # what a run killed after step 5 would have left behind
        f.write(json.dumps({"step": 4, "loss": 0.0}) + "\n" + json.dumps({"step": 5, "loss": 0.0}) + "\n")
    cfg2 = rt.mode0_cfg(toys / "toys", toys / name, "--log.auto_resume", "true", *extra)
    coach2 = rt.coach(cfg2, seed=77)
    assert coach2.start_step == 3 and rt.train_counting(coach2) == 3
    rt.assert_end(end_a, rt.end_state(coach2))
    assert _metrics(cfg2) == text, "the resumed run's record differs from the uninterrupted one"


def test_coach_record_is_deterministic_and_continues_across_a_resume(toys, run_u):
    cfg_a, end_a, text = run_u
    _check_lines(text, clipped=False)
    _, end_b, text_b = _run6(toys, "ub", ())
    assert text == text_b, "two runs of one configuration write different records"
    rt.assert_end(end_a, end_b)
    log = (cfg_a.log.logging_dir / "log.txt").read_text()
    assert "grad_norm" in log and "loss_scale" in log
    ck = torch.load(cfg_a.log.exp_dir / "mapper-steps-3_object.pt", map_location="cpu", weights_only=False)
    assert "train_metrics" not in ck["cfg"]["log"] and "max_grad_norm" not in ck["cfg"]["optim"]
    assert not any("max_grad_norm" in k or "train_metrics" in k for k in ck["vneti_ext"]["config_ext"])
    _check_resume(toys, "ur", (), cfg_a, end_a, text)
    # a state saved without clipping is refused by a clipped run, and the field is named
    cfg3 = rt.mode0_cfg(toys / "toys", toys / "ux", "--model.mapper_checkpoint_path",
                         str(cfg_a.log.exp_dir / "mapper-steps-3"), "--optim.max_grad_norm", "0.05")
    with pytest.raises(ValueError, match="max_grad_norm"):
        rt.coach(cfg3)


def test_coach_clipped_run_resumes_and_is_told_apart(toys, run_u):
    """max_grad_norm = half the first step's norm of the unclipped run"""
    cfg_u, end_u, text_u = run_u
    bound = repr(0.5 * json.loads(text_u.decode().splitlines()[0])["grad_norm"]["total"])
    clip = ("--optim.max_grad_norm", bound)
    cfg_a, end_a, text = _run6(toys, "ca", clip)
    lines = _check_lines(text, clipped=True)
    assert lines[0]["clip_coef"] == pytest.approx(0.5, rel=1e-3)
    assert not torch.equal(end_a["params"], end_u["params"]), "clipping must change the training"
    ck = torch.load(cfg_a.log.exp_dir / "mapper-steps-3_object.pt", map_location="cpu", weights_only=False)
    assert "max_grad_norm" not in ck["cfg"]["optim"] and ck["vneti_ext"]["config_ext"]["optim.max_grad_norm"] == float(bound)
    _check_resume(toys, "cr", clip, cfg_a, end_a, text)
    # and the reverse: a clipped run's state is refused by an unclipped run
    cfg3 = rt.mode0_cfg(toys / "toys", toys / "cx", "--model.mapper_checkpoint_path", str(cfg_a.log.exp_dir / "mapper-steps-3"))
    with pytest.raises(ValueError, match="max_grad_norm"):
        rt.coach(cfg3)
