"""Resumable training on the GPU: `TrainStepEngine.state_dict / load_state_dict`, the autotuner picks as data, and
`Coach` continuing from `model.mapper_checkpoint_path` / `log.auto_resume` (tiny SD shape family, batch 2).

Every comparison is for BIT equality (torch.equal): a resumed run replays the same graphs on the same state with the same
picks, so there is no tolerance to choose."""
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from helpers.coach_runs import assert_end as _assert_end, coach as _coach, end_state as _end_state
from helpers.coach_runs import mapper_tensors as _mapper_tensors, mode0_cfg as _mode0_cfg, toys as _toys
from helpers.coach_runs import train_counting as _train
from helpers.engines import FIELDS, build_device_rng_engine, feed_device_rng, run_steps, snapshot

pytestmark = pytest.mark.gpu

B, H, W, LR = 2, 64, 64, 3e-3
ACCUM = 2
SCENES = [0, 2, 0, 2]
N_IMAGES = 4


# ------------------------------------------------------------------------------------------------ engine level
def _build(mode3=False, cache=0):
    """accumulation 2 on top of the device-RNG form: a GradScaler mid-count after 2 steps, doubling inside steps 3-4"""
    return build_device_rng_engine(mode3, ACCUM, B, H, W, LR, moment_cache_images=cache)


def _feed(cfg, eng, step, micro, mode3):
    feed_device_rng(cfg, eng, step, micro, mode3, scenes=SCENES, stride=ACCUM, n_images=N_IMAGES)


def _steps(cfg, eng, steps, mode3):
    run_steps(cfg, eng, steps, mode3, _feed)


def _record(eng):
    rec = snapshot(eng, FIELDS)
    rec["loss"] = eng.loss()
    return rec


def _assert_same(want, got, what):
    for f in FIELDS:
        assert torch.equal(want[f], got[f]), f"{what}: {f} differs"
    assert want["loss"] == got["loss"], f"{what}: loss {want['loss']!r} vs {got['loss']!r}"


_REF = {}


def _reference(mode3, cache):
    """computed once per engine form and left unchanged: the state after 2 optimizer steps, the record after 4 (one
    uninterrupted captured run), and the engine itself for the in-place test"""
    key = (mode3, cache)
    if key not in _REF:
        cfg, eng = _build(mode3, cache)
        _feed(cfg, eng, 0, 0, mode3)
        eng.capture()
        _steps(cfg, eng, (0, 1), mode3)
        sd = eng.state_dict()
        _steps(cfg, eng, (2, 3), mode3)
        _REF[key] = (cfg, eng, sd, _record(eng))
    return _REF[key]


def test_engine_state_reloads_in_place_after_capture():
    cfg, eng, sd, want = _reference(False, 0)
    assert all(not t.is_cuda for t in sd.values() if torch.is_tensor(t)) and sd["meta"]["grad_accum"] == ACCUM
    # the state is non-trivial where it was taken and moves inside the compared window
    assert int(sd["opt_step"]) == 2 and float(sd["scaler"][1]) == 2.0, sd["scaler"]
    assert float(want["scaler"][0]) == 2 * float(sd["scaler"][0]), "the loss scale must double inside the window"
    assert not torch.equal(sd["rng_state"], want["rng_state"]) and float(sd["exp_avg_sq"].abs().max()) > 0
    n_launches = len(eng.launches())
    graph = eng.graph_a
    eng.load_state_dict(sd)
    assert eng.graph_a is graph and len(eng.launches()) == n_launches, "no re-capture, same launch list"
    for f in FIELDS:
        assert torch.equal(getattr(eng, f).cpu(), sd[f]), f
    _steps(cfg, eng, (2, 3), False)
    _assert_same(want, _record(eng), "in-place reload")
    # legal only between optimizer steps
    _feed(cfg, eng, 4, 0, False)
    assert eng.step() is False
    with pytest.raises(RuntimeError, match="accumulation"):
        eng.state_dict()
    with pytest.raises(RuntimeError, match="accumulation"):
        eng.load_state_dict(sd)
    _feed(cfg, eng, 4, 1, False)
    assert eng.step() is True
    # a state that does not fit names every mismatch
    bad = dict(sd, meta=dict(sd["meta"], grad_accum=1, precision="bf16"), params=sd["params"][:-1])
    with pytest.raises(ValueError) as err:
        eng.load_state_dict(bad)
    assert all(k in str(err.value) for k in ("grad_accum", "precision", "params"))


@pytest.mark.parametrize("mode3,cache", [(False, 0), (True, 0), (False, N_IMAGES)], ids=["one-mapper", "mode3", "moment-cache"])
def test_engine_state_loads_into_a_fresh_engine_before_capture(mode3, cache):
    """the load survives `_capture`'s warm-up snapshot; the fresh engine's moment cache starts empty and refills (D14: a hit
    and a miss are bit-identical)"""
    cfg, ref_eng, sd, want = _reference(mode3, cache)
    _, eng = _build(mode3, cache)
    assert eng is not ref_eng and not torch.equal(eng.params.cpu(), sd["params"])
    eng.load_state_dict(sd)
    _feed(cfg, eng, 2, 0, mode3)
    eng.capture()
    assert torch.equal(eng.params.cpu(), sd["params"]) and torch.equal(eng.rng_state.cpu(), sd["rng_state"])
    _steps(cfg, eng, (2, 3), mode3)
    _assert_same(want, _record(eng), "fresh engine")
    if mode3:
        # torch's per-parameter step counts: a mapper counts from its first gradient on (scenes 0, 2, 0, 2; mapper 1 never)
        assert sd["seg_step"].tolist() == [2, 0, 1] and want["seg_step"].tolist() == [4, 0, 3]
    if cache:
        assert sorted(eng._cached_images) == list(range(N_IMAGES)) and eng.graph_a_c is not None
    # an engine of another form refuses the state
    if mode3:
        with pytest.raises(ValueError, match="n_objects"):
            _reference(False, 0)[1].load_state_dict(sd)


def test_autotuner_picks_export_and_preload():
    from view_neti_amd.engine import schedule as S
    _reference(False, 0)
    cache = S.Schedule._tile_cache
    before = dict(cache)
    assert before, "the engine above pinned its picks"
    data = S.export_picks()
    assert set(data) == {"kernel_tree_sha", "picks"} and len(data["picks"]) == len(before)
    try:
        cache.clear()
        assert S.preload_picks(data) is True
        assert cache == before
        _build(False, 0)
        assert cache == before, "an engine built after the preload must find every problem pinned"
        cache.clear()
        assert S.preload_picks(dict(data, kernel_tree_sha="0" * 16)) is False and not cache
    finally:
        cache.clear()
        cache.update(before)


# ------------------------------------------------------------------------------------------------ Coach
@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """the uninterrupted run: 6 optimizer steps, checkpoints and trainer states at 3 and 6"""
    tmp = tmp_path_factory.mktemp("resume")
    _toys(tmp / "toys")
    cfg = _mode0_cfg(tmp / "toys", tmp / "a")
    coach = _coach(cfg)
    assert coach.start_step == 0 and _train(coach) == 6
    out = cfg.log.exp_dir
    for name in ("mapper-steps-3_object.pt", "trainer-state-steps-3.pt", "mapper-steps-6_object.pt",
                 "trainer-state-steps-6.pt", "mapper-final_object.pt"):
        assert (out / name).exists(), name
    assert not [f.name for f in out.iterdir() if f.name.endswith(".tmp")]
    return dict(tmp=tmp, toys=tmp / "toys", out=out, end=_end_state(coach))


def test_coach_exact_resume(run_a):
    from view_neti_amd.compat import resume as R
    state = torch.load(run_a["out"] / "trainer-state-steps-3.pt", weights_only=True)
    assert state["step"] == 3 and int(state["engine"]["opt_step"]) == 3 and state["host"]["sampler"]["pos"] == 6
    cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "b", "--model.mapper_checkpoint_path",
                     str(run_a["out"] / "mapper-steps-3"))
    coach = _coach(cfg, seed=4321)  # other host streams than run A's: the restored ones must take over
    assert coach.start_step == 3 and int(coach.engine.opt_step) == 3
    assert float(coach.engine.hyper[0]) == float(np.float32(coach.lr_schedule.lr(3)))
    assert _train(coach) == 3
    _assert_end(run_a["end"], _end_state(coach))
    a, b = _mapper_tensors(run_a["out"] / "mapper-final_object.pt"), _mapper_tensors(cfg.log.exp_dir / "mapper-final_object.pt")
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # B saved its own state at step 6, equal to A's in every engine tensor
    sa = R.load_state(run_a["out"] / "trainer-state-steps-6.pt")["engine"]
    sb = R.load_state(cfg.log.exp_dir / "trainer-state-steps-6.pt")["engine"]
    assert all(torch.equal(sa[f], sb[f]) for f in FIELDS)


def test_coach_warm_start(run_a):
    from view_neti_amd.compat.checkpoint_handler import CheckpointHandler
    from view_neti_amd.engine.text import flatten_mapper_state
    src = run_a["tmp"] / "pair_only"
    src.mkdir()
    shutil.copy(run_a["out"] / "mapper-steps-3_object.pt", src / "mapper-steps-3_object.pt")
    cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "warm", "--model.mapper_checkpoint_path",
                     str(src / "mapper-steps-3_object.pt"))
    coach = _coach(cfg)
    log = (cfg.log.logging_dir / "log.txt").read_text()
    assert log.count("WARNING: warm start") == 1 and "trainer-state-steps-3.pt" in log
    eng = coach.engine
    tid = coach.placeholder_object_token_ids[0]
    _, lookup = CheckpointHandler.load_mapper(src / "mapper-steps-3_object.pt", "object", ["<toy>"], [tid])
    assert torch.equal(eng.params.cpu(), flatten_mapper_state(lookup[tid].mapper_state()))
    assert coach.start_step == 3 and int(eng.opt_step) == 0 and int(eng.seg_step.abs().max()) == 0
    assert float(eng.exp_avg.abs().max()) == 0.0 and float(eng.exp_avg_sq.abs().max()) == 0.0
    assert eng.scaler.tolist() == [65536.0, 0.0, 0.0]
    assert float(eng.hyper[0]) == float(np.float32(coach.lr_schedule.lr(3)))
    assert _train(coach) == 3
    end = _end_state(coach)
    assert torch.isfinite(end["params"]).all() and torch.isfinite(end["exp_avg_sq"]).all() and int(end["opt_step"]) == 3
    assert not torch.equal(end["params"], run_a["end"]["params"]), "a warm start is not the interrupted run"


def test_coach_auto_resume(run_a):
    out = run_a["tmp"] / "auto"
    cfg = _mode0_cfg(run_a["toys"], out, "--log.auto_resume", "true")
    coach = _coach(cfg)
    assert coach.start_step == 0, "an empty directory starts at 0"
    assert "no complete trainer state" in (cfg.log.logging_dir / "log.txt").read_text()
    # pre-empted after step 3: the schedule is the 6-step one, the loop is cut short
    cfg.optim.max_train_steps = 3
    assert _train(coach) == 3 and (cfg.log.exp_dir / "trainer-state-steps-3.pt").exists()
    del coach
    # relaunched with the same command line
    cfg2 = _mode0_cfg(run_a["toys"], out, "--log.auto_resume", "true")
    coach2 = _coach(cfg2, seed=77)
    assert coach2.start_step == 3
    assert _train(coach2) == 3
    _assert_end(run_a["end"], _end_state(coach2))
    names = sorted(f.name for f in cfg2.log.exp_dir.iterdir() if f.name.startswith("trainer-state"))
    assert names == ["trainer-state-steps-3.pt", "trainer-state-steps-6.pt"]


def test_coach_refusals(run_a):
    from view_neti_amd.compat.coach import Coach
    cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "w2", "--data.dataloader_num_workers", "2")
    with pytest.raises(ValueError, match="dataloader_num_workers"):
        Coach(cfg)
    cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "w2r", "--data.dataloader_num_workers", "2", "--log.save_trainer_state",
                     "false", "--model.mapper_checkpoint_path", str(run_a["out"] / "mapper-steps-3"))
    with pytest.raises(ValueError, match="dataloader_num_workers"):
        Coach(cfg)
    cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "bs", "--optim.train_batch_size", "1", "--model.mapper_checkpoint_path",
                     str(run_a["out"] / "mapper-steps-3"))
    with pytest.raises(ValueError, match="train_batch_size"):
        Coach(cfg)
    for bad in ("mapper-final", "mapper-steps-4"):
        cfg = _mode0_cfg(run_a["toys"], run_a["tmp"] / "nf", "--model.mapper_checkpoint_path", str(run_a["out"] / bad))
        with pytest.raises((ValueError, FileNotFoundError)):
            Coach(cfg)


M3_YAML = """
learnable_mode: 3
log: {{exp_name: m3, exp_dir: {out}, save_steps: 3, save_trainer_state: true}}
data: {{train_data_dir: data/dtu/Rectified, train_data_subsets: [scan65, scan125], super_category_object_tokens: [object, object],
       placeholder_object_tokens: [<skull>, <statue>], placeholder_object_token: <object>, dataloader_num_workers: 0,
       camera_representation: dtu-12d, dtu_subset: 3, dtu_lighting: 3, dtu_preprocess_key: 0, augmentation_key: 0,
       resolution: 64}}
model: {{arch_mlp_hidden_dims: 128, use_nested_dropout: True, nested_dropout_prob: 0.5, word_embedding_dim: 128,
        arch_view_net: 15, arch_view_disable_tl: False, pe_sigma_exp_key: 2, output_bypass_alpha_view: 5,
        output_bypass_alpha_object: 5, bypass_unconstrained_view: True{resume}}}
eval: {{validation_seeds: [0, 1], num_validation_images: 2, eval_placeholder_object_tokens: [<skull>]}}
optim: {{max_train_steps: 6, train_batch_size: 2, gradient_accumulation_steps: 1, mixed_precision: fp16}}
"""


def test_coach_mode3_exact_resume(tmp_path, monkeypatch):
    """the two-scene layout of test_coach_mode3_multi_scene: the scene sequence (numpy's global stream across
    `reset_sampled_object`), the per-mapper step counts and the end state continue exactly"""
    from view_neti_amd.compat import config as C
    from view_neti_amd.compat.dataset import TextualInversionDataset
    monkeypatch.chdir(tmp_path)
    cal = tmp_path / "data" / "dtu" / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    rng = np.random.RandomState(1)
    mats = rng.randn(49, 3, 4) * np.array([[1e3, 1e3, 1e3, 1e5]])
    for i in range(49):
        np.savetxt(cal / f"pos_{i + 1:03d}.txt", mats[i])
    for scan in ("scan65", "scan125"):
        d = tmp_path / "data" / "dtu" / "Rectified" / scan
        d.mkdir(parents=True)
        for c in TextualInversionDataset.dtu_get_train_idxs(3):  # the three training views of dtu_subset 3
            Image.fromarray(rng.randint(0, 255, (120, 160, 3), dtype=np.uint8)).save(
                d / TextualInversionDataset.dtu_cam_and_lighting_to_fname(c, "3"))

    def run(name, resume_from=None, seed=0):
        y = tmp_path / f"{name}.yaml"
        extra = f", mapper_checkpoint_path: {resume_from}" if resume_from else ""
        y.write_text(M3_YAML.format(out=str(tmp_path / name), resume=extra))
        cfg = C.parse(C.RunConfig, ["--config_path", str(y)])
        cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
        cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
        coach = _coach(cfg, seed)
        scenes, orig = [], coach.engine.set_batch

        def spy(*a, **k):
            scenes.append(k["object_index"])
            return orig(*a, **k)
        coach.engine.set_batch = spy
        steps = _train(coach)
        return cfg, coach, scenes, steps

    cfg_a, a, scenes_a, steps_a = run("a")
    assert steps_a == 6 and len(scenes_a) == 6 and set(scenes_a) == {0, 1}, scenes_a
    cfg_b, b, scenes_b, steps_b = run("b", cfg_a.log.exp_dir / "mapper-steps-3_view.pt", seed=99)
    assert b.start_step == 3 and steps_b == 3
    assert scenes_b == scenes_a[3:], f"scene sequence {scenes_b} after the resume, {scenes_a[3:]} uninterrupted"
    end_a, end_b = _end_state(a), _end_state(b)
    _assert_end(end_a, end_b)
    assert int(end_a["seg_step"].min()) > 0 and int(end_a["seg_step"].max()) == 6 - min(scenes_a.index(0), scenes_a.index(1))
    for kind in ("object", "view"):
        ta = _mapper_tensors(cfg_a.log.exp_dir / f"mapper-final_{kind}.pt")
        tb = _mapper_tensors(cfg_b.log.exp_dir / f"mapper-final_{kind}.pt")
        assert list(ta) == list(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
