"""Host side of resumable training (view_neti_amd/compat/resume.py): the batch sampler against the stock shuffling
DataLoader draw for draw, host-state round trips through the real dataset in the middle of an epoch, checkpoint names,
latest-complete selection, retention, the atomic write, the fingerprint and the lr schedule after a resume.
Every comparison is for equality."""
import random

import numpy as np
import pytest
import torch
from PIL import Image
from torch.utils.data import DataLoader

from view_neti_amd.compat import resume as R
from view_neti_amd.compat.dataset import TextualInversionDataset
from view_neti_amd.compat.lr_schedule import LRSchedule
from view_neti_amd.compat.tokenizer import HashTokenizer


# ------------------------------------------------------------------------------------------------ 1. order parity
class _Items(torch.utils.data.Dataset):
    def __init__(self, n, draws):
        self.n, self.draws = n, draws

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        # `draws`: the item consumes the global generator, like the augmentations of the real dataset
        return torch.tensor([float(i), float(torch.rand(1)) if self.draws else 0.0])


def _epochs(loader, n_epochs):
    return [[b.clone() for b in loader] for _ in range(n_epochs)]


@pytest.mark.parametrize("n", [7, 6])
@pytest.mark.parametrize("explicit,draws", [(False, False), (True, False), (False, True), (True, True)])
def test_batch_sampler_reproduces_the_shuffling_loader(n, explicit, draws):
    ds = _Items(n, draws)

    def gen():
        return torch.Generator().manual_seed(11) if explicit else None

    torch.manual_seed(5)
    g0 = gen()
    want = _epochs(DataLoader(ds, batch_size=2, shuffle=True, drop_last=True, generator=g0), 3)
    end0 = (torch.get_rng_state(), g0.get_state() if explicit else None)
    torch.manual_seed(5)
    g1 = gen()
    sampler = R.ResumableBatchSampler(n, 2, generator=g1)
    got = _epochs(DataLoader(ds, batch_sampler=sampler, generator=g1), 3)
    end1 = (torch.get_rng_state(), g1.get_state() if explicit else None)
    assert [len(e) for e in got] == [n // 2] * 3 == [len(e) for e in want]
    for ew, eg in zip(want, got):
        for bw, bg in zip(ew, eg):
            assert torch.equal(bw, bg)
    # the streams end where the stock loader leaves them (the discarded tail permutation advances an explicit generator)
    assert torch.equal(end0[0], end1[0])
    if explicit:
        assert torch.equal(end0[1], end1[1])
    assert sampler.epoch == 3 and sampler.pos == n // 2 and sorted(sampler.order.tolist()) == list(range(n))


# ------------------------------------------------------------------------------------------------ 2 / 3. round trips
def _drive(loader, sampler, ds, n_batches, snapshot_after=None, restore=None, gen=None, mode3=False):
    """the shape of Coach.train's loop: one loader iterator per epoch; the restore goes in after the iterator exists"""
    out, snap = [], None
    while len(out) < n_batches:
        it = iter(loader)
        if restore is not None:
            R.restore_host_state(restore, sampler, ds, gen)
            restore = None
        for b in it:
            out.append(b)
            if mode3:
                ds.reset_sampled_object()
            if len(out) == snapshot_after:
                snap = R.capture_host_state(sampler, ds, gen)
            if len(out) >= n_batches:
                break
    return out, snap


def _through_file(state, path):
    torch.save(state, path)
    return torch.load(path, weights_only=True)


def _same(a, b, keys=("input_ids", "image_idx", "pixel_values", "input_ids_placeholder_object")):
    return a["text"] == b["text"] and all(torch.equal(a[k], b[k]) for k in keys)


def _disturb():
    torch.manual_seed(999)
    np.random.seed(999)
    random.seed(999)


@pytest.mark.parametrize("explicit", [False, True])
def test_host_state_round_trip_mid_epoch(tmp_path, explicit):
    root = tmp_path / "toys"
    root.mkdir()
    rng = np.random.RandomState(0)
    for i in range(5):
        Image.fromarray(rng.randint(0, 255, (40, 48, 3), dtype=np.uint8)).save(root / f"{i}.png")
    tk = HashTokenizer()
    tk.add_tokens(["<toy>"])

    def build():
        ds = TextualInversionDataset(root, tk, learnable_mode=0, size=32, repeats=1, placeholder_object_token="<toy>",
                                     augmentation_key=5)
        gen = torch.Generator().manual_seed(3) if explicit else None
        sampler = R.ResumableBatchSampler(len(ds), 2, generator=gen)
        return ds, gen, sampler, DataLoader(ds, batch_sampler=sampler, generator=gen,
                                            collate_fn=TextualInversionDataset.collate)

    torch.manual_seed(1)
    np.random.seed(1)
    random.seed(1)
    ds, gen, sampler, loader = build()
    full, snap = _drive(loader, sampler, ds, 7, snapshot_after=3, gen=gen)
    assert snap["sampler"]["epoch"] == 2 and snap["sampler"]["pos"] == 1  # 2 batches per epoch: inside the second epoch
    assert len({b["text"][0] for b in full}) > 1 and not torch.equal(full[0]["pixel_values"], full[2]["pixel_values"])
    snap = _through_file(snap, tmp_path / "host.pt")
    ds, gen, sampler, loader = build()
    _disturb()
    rest, _ = _drive(loader, sampler, ds, 4, restore=snap, gen=gen)
    for k in range(4):
        assert _same(full[3 + k], rest[k]), f"batch {4 + k} differs after the restore"
    with pytest.raises(ValueError, match="generator"):
        R.restore_host_state(snap, sampler, ds, None if explicit else torch.Generator())


@pytest.mark.parametrize("snapshot_after", [3, 4])  # 3 batches per epoch: at the very end of epoch 1 / inside epoch 2
def test_host_state_round_trip_mode3(tmp_path, monkeypatch, snapshot_after):
    monkeypatch.chdir(tmp_path)
    cal = tmp_path / "data" / "dtu" / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    rng = np.random.RandomState(1)
    mats = rng.randn(49, 3, 4) * np.array([[1e3, 1e3, 1e3, 1e5]])
    for i in range(49):
        np.savetxt(cal / f"pos_{i + 1:03d}.txt", mats[i])
    scans = ["scan65", "scan125"]
    for scan in scans:
        d = tmp_path / "data" / "dtu" / "Rectified" / scan
        d.mkdir(parents=True)
        for c in range(49):
            Image.fromarray(rng.randint(0, 255, (30, 40, 3), dtype=np.uint8)).save(
                d / TextualInversionDataset.dtu_cam_and_lighting_to_fname(c, "3"))
    tk = HashTokenizer()

    def build():
        ds = TextualInversionDataset("data/dtu/Rectified", tk, camera_representation="dtu-12d", learnable_mode=3,
                                     train_data_subsets=scans, placeholder_object_tokens=["<skull>", "<statue>"],
                                     dtu_subset=3, dtu_lighting=3, dtu_preprocess_key=1, repeats=1,
                                     placeholder_object_token="<object>")
        tk.add_tokens(ds.placeholder_tokens)
        sampler = R.ResumableBatchSampler(len(ds), 2)
        return ds, sampler, DataLoader(ds, batch_sampler=sampler, collate_fn=TextualInversionDataset.collate)

    torch.manual_seed(2)
    np.random.seed(4)
    random.seed(2)
    ds, sampler, loader = build()
    assert len(ds) == 6
    full, snap = _drive(loader, sampler, ds, 7, snapshot_after=snapshot_after, mode3=True)
    scenes = [int(b["input_ids_placeholder_object"][0]) for b in full]
    assert len(set(scenes)) == 2, f"the scene sampler never switched: {scenes}"
    assert snap["current_object_idx"] in (0, 1) and snap["sampler"]["pos"] == (3 if snapshot_after == 3 else 1)
    snap = _through_file(snap, tmp_path / "host.pt")
    ds, sampler, loader = build()
    _disturb()
    ds.current_object_idx = 1 - snap["current_object_idx"]
    n_rest = 7 - snapshot_after
    rest, _ = _drive(loader, sampler, ds, n_rest, restore=snap, mode3=True)
    for k in range(n_rest):
        assert _same(full[snapshot_after + k], rest[k], keys=("input_ids", "image_idx", "pixel_values",
                                                             "input_ids_placeholder_object",
                                                             "input_ids_placeholder_view")), f"batch {snapshot_after + k + 1}"


# ------------------------------------------------------------------------------------------------ 4. names and files
def test_checkpoint_names(tmp_path):
    for name in ("mapper-steps-250", "mapper-steps-250_object.pt", "mapper-steps-250_view.pt"):
        assert R.parse_step(tmp_path / name) == 250
    for name in ("mapper-final", "mapper-final_object.pt", "mapper-steps-x", "mapper-steps-", "mapper-steps-3_view",
                 "learned_embeds-steps-3.bin", "trainer-state-steps-3.pt"):
        with pytest.raises(ValueError, match="not a step checkpoint"):
            R.parse_step(tmp_path / name)
    assert [f.name for f in R.resume_files(tmp_path, 7, 3, world=2)] == [
        "mapper-steps-7_object.pt", "mapper-steps-7_view.pt", "trainer-state-steps-7.pt",
        "trainer-state-steps-7.host-rank1.pt"]
    assert list(R.mapper_files(tmp_path, 7, 1)) == ["view"] and list(R.mapper_files(tmp_path, 7, 0)) == ["object"]
    assert list(R.mapper_files(tmp_path, 7, 5)) == ["object"] and list(R.mapper_files(tmp_path, 7, 2)) == ["object", "view"]
    with pytest.raises(FileNotFoundError, match="mapper-steps-7_object.pt"):
        R.resolve_checkpoint(tmp_path / "mapper-steps-7", 0)
    (tmp_path / "mapper-steps-7_object.pt").write_bytes(b"x")
    for spelling in ("mapper-steps-7", "mapper-steps-7_object.pt", "mapper-steps-7_view.pt"):
        assert R.resolve_checkpoint(tmp_path / spelling, 0) == (tmp_path, 7)
    with pytest.raises(FileNotFoundError, match="mapper-steps-7_view.pt"):  # mode 2 trains the view mapper too
        R.resolve_checkpoint(tmp_path / "mapper-steps-7", 2)


def _fake_state(step):
    return {"format": R.FORMAT, "step": step, "engine": {"params": torch.arange(4096, dtype=torch.float32) + step}}


def test_latest_complete_retention_and_atomic_write(tmp_path):
    assert R.latest_complete_state(tmp_path / "nowhere", 0) is None and R.latest_complete_state(tmp_path, 0) is None
    for step in (3, 6, 9, 12):
        (tmp_path / f"mapper-steps-{step}_object.pt").write_bytes(b"x")
        R.atomic_save(_fake_state(step), R.state_file(tmp_path, step))
    assert R.list_states(tmp_path) == [3, 6, 9, 12] and R.latest_complete_state(tmp_path, 0) == 12
    assert not [f.name for f in tmp_path.iterdir() if "tmp" in f.name], "the atomic write left its temporary file behind"
    # a save cut short: the newest state holds half its bytes -> the one before it
    newest = R.state_file(tmp_path, 12)
    blob = newest.read_bytes()
    newest.write_bytes(blob[:len(blob) // 2])
    assert R.latest_complete_state(tmp_path, 0) == 9
    # mode 2 needs the view checkpoint too; two ranks need rank 1's host file
    assert R.latest_complete_state(tmp_path, 2) is None
    (tmp_path / "mapper-steps-6_view.pt").write_bytes(b"x")
    assert R.latest_complete_state(tmp_path, 2) == 6
    assert R.latest_complete_state(tmp_path, 0, world=2) is None
    R.atomic_save(_fake_state(3), R.state_file(tmp_path, 3, rank=1))
    assert R.latest_complete_state(tmp_path, 0, world=2) == 3
    # a write that fails leaves neither the final name nor the temporary file
    with pytest.raises(Exception):
        R.atomic_save({"f": lambda: 0}, tmp_path / "trainer-state-steps-15.pt")
    assert R.list_states(tmp_path) == [3, 6, 9, 12] and not [f for f in tmp_path.iterdir() if "tmp" in f.name]
    # retention: exactly `keep` states stay, host-rank files go with their state, mapper checkpoints are never removed
    assert R.prune_states(tmp_path, 0) == []
    removed = R.prune_states(tmp_path, 2)
    assert sorted(f.name for f in removed) == ["trainer-state-steps-3.host-rank1.pt", "trainer-state-steps-3.pt",
                                               "trainer-state-steps-6.pt"]
    assert R.list_states(tmp_path) == [9, 12]
    assert all((tmp_path / f"mapper-steps-{s}_object.pt").exists() for s in (3, 6, 9, 12))


# ------------------------------------------------------------------------------------------------ 5. state file safety
def test_state_file_is_plain_data_and_fingerprint_names_mismatches(tmp_path):
    sampler = R.ResumableBatchSampler(6, 2, generator=torch.Generator().manual_seed(0))
    next(iter(sampler))
    fp = R.fingerprint(learnable_mode=3, batch_size=2, grad_accum=2, world=1, precision="fp16", seed=0, dataset_len=600,
                       n_params=123456)
    state = {"format": R.FORMAT, "step": 3, "fingerprint": fp,
             "engine": {"params": torch.randn(8), "opt_step": torch.tensor([3], dtype=torch.int32),
                        "meta": {"n_params": 8, "view_in_bucket": True, "precision": "fp16"}},
             "picks": {"kernel_tree_sha": "0123456789abcdef", "picks": {repr((64, 64, 64, 1, None, False, 0)): [3, 1, 0]}},
             "host": R.capture_host_state(sampler, None, sampler.generator)}
    path = R.state_file(tmp_path, 3)
    R.atomic_save(state, path)
    back = torch.load(path, weights_only=True)  # no pickled objects: the restricted loader takes it
    assert back["fingerprint"] == fp and back["picks"] == state["picks"] and back["host"]["sampler"]["pos"] == 1
    assert torch.equal(back["host"]["torch"], state["host"]["torch"]) and R.load_state(path)["step"] == 3
    R.check_fingerprint(back["fingerprint"], fp)
    R.check_fingerprint(back["fingerprint"], {k: v for k, v in fp.items() if k != "n_params"})  # the early, partial check
    other = R.fingerprint(learnable_mode=3, batch_size=4, grad_accum=2, world=2, precision="bf16", seed=0, dataset_len=600,
                          n_params=123456)
    with pytest.raises(ValueError) as err:
        R.check_fingerprint(back["fingerprint"], other)
    msg = str(err.value)
    assert all(k in msg for k in ("train_batch_size", "world_size", "precision"))
    assert not any(k in msg for k in ("learnable_mode", "gradient_accumulation_steps", "seed", "dataset_len", "n_params"))
    torch.save({"format": 0}, tmp_path / "old.pt")
    with pytest.raises(ValueError, match="not a trainer state"):
        R.load_state(tmp_path / "old.pt")


# ------------------------------------------------------------------------------------------------ 6. lr schedule
@pytest.mark.parametrize("name,warmup", [("cosine", 2), ("constant", 0)])
def test_lr_after_resume_is_the_uninterrupted_value(name, warmup):
    args = (name, 4e-3, warmup, 10, 2, 1)
    uninterrupted = [LRSchedule(*args).lr(g) for g in range(11)]
    for n in (0, 1, 3, 7, 10):
        assert LRSchedule(*args).lr(n) == uninterrupted[n]  # a pure function of the step count: nothing to restore
    if name == "cosine":
        # warm-up counts micro-iterations (2 steps x accumulation 2), the scheduler advances once per optimizer step
        assert uninterrupted[0] == 0.0 and uninterrupted[2] == 2e-3 and uninterrupted[4] == 4e-3 > uninterrupted[5]


# ------------------------------------------------------------------------------------------------ scripts/train.py
def test_train_script_accepts_an_existing_directory_only_to_continue_it(tmp_path):
    from scripts.train import prepare_directories
    from view_neti_amd.compat import config as C
    (tmp_path / "run0").mkdir()
    args = ["--log.exp_dir", str(tmp_path), "--log.exp_name", "run0"]
    with pytest.raises(ValueError, match="already exists"):
        prepare_directories(C.parse(C.RunConfig, args))
    cfg = C.parse(C.RunConfig, args + ["--log.auto_resume", "true"])
    prepare_directories(cfg)
    assert cfg.log.exp_dir == tmp_path / "run0" and cfg.log.logging_dir == tmp_path / "run0" / "logs"
    # run control stays out of checkpoints and out of the config.yaml of runs that do not use it
    assert "log.auto_resume" not in C.ext_fields(cfg) and C.encode(cfg)["log"]["auto_resume"] is True
    plain = C.encode(C.parse(C.RunConfig, args))["log"]
    assert not {"save_trainer_state", "keep_trainer_states", "auto_resume"} & set(plain)
