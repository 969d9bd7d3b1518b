"""Host side of the object-masked diffusion loss, `data.mask_dir`: the float64 restatement the
GPU tests compare against (tests/helpers/loss_mask_ref.py), the geometric part of an augmentation plan, the data set's
masks, the configuration fields, the resume fingerprint and the `masked` mark of train-metrics.jsonl.  No GPU."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from helpers import loss_mask_ref as MR

from view_neti_amd.compat import augment as A
from view_neti_amd.compat import config as C
from view_neti_amd.compat import resume as R
from view_neti_amd.compat import train_metrics as TM
from view_neti_amd.compat.dataset import TextualInversionDataset
from view_neti_amd.compat.tokenizer import HashTokenizer


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("H,W,f", [(8, 8, 8), (24, 40, 8), (136, 248, 8), (12, 20, 4)])
@pytest.mark.parametrize("bg", [0.0, 0.25])
def test_weights_against_a_direct_torch_evaluation(H, W, f, bg):
    mask = MR.random_mask(H, W, seed=H + W)
    q = MR.weights_from_mask(mask, f, 3, bg)
    m = bg + (1.0 - bg) * F.avg_pool2d(((mask.double() / 255.0) > 0.01).double()[None, None], f)[0, 0].reshape(-1)
    want = m * m.numel() / m.sum()
    assert q.dtype == torch.float64 and q.shape == ((H // f) * (W // f),)
    assert torch.allclose(q, want, rtol=1e-13, atol=0)
    assert q.mean().item() == pytest.approx(1.0, rel=1e-13)
    # the threshold is `mask / 255 > 0.01` on uint8: 2 is background, 3 is foreground
    assert torch.equal(MR.cell_counts(torch.tensor([[2, 3], [3, 2]], dtype=torch.uint8), 2), torch.tensor([[2]]))


def test_loss_is_the_per_sample_normalised_masked_mse():
    g = torch.Generator().manual_seed(0)
    B, Cc, h, w, f = 3, 4, 3, 5, 8
    masks = [MR.random_mask(h * f, w * f, seed=10 + b) for b in range(B)]
    for bg in (0.0, 0.25):
        q = torch.stack([MR.weights_from_mask(m, f, 3, bg) for m in masks])
        pred = torch.randn(B, Cc, h * w, generator=g, dtype=torch.float64, requires_grad=True)
        target = torch.randn(B, Cc, h * w, generator=g, dtype=torch.float64)
        wb = torch.tensor([0.5, 1.0, 0.125], dtype=torch.float64)
        for wts in (None, wb):
            loss, grad = MR.weighted_loss(pred, target, q, wts)
            # explicit: every sample's masked squared error over (channels x its own mask mass), then the batch mean
            d2 = (pred - target) ** 2
            per = []
            for b in range(B):
                m = bg + (1.0 - bg) * MR.cell_counts(masks[b], f).reshape(-1).double() / (f * f)
                per.append((m * d2[b]).sum() / (Cc * m.sum()))
            per = torch.stack(per)
            want = (per * (wb if wts is not None else 1.0)).mean()
            assert loss.item() == pytest.approx(want.item(), rel=1e-13)
            (g_auto,) = torch.autograd.grad(loss, pred)
            assert torch.allclose(g_auto, grad, rtol=1e-12, atol=0)
            if wts is None:
                assert torch.allclose(MR.per_sample(pred, target, q), per, rtol=1e-13, atol=0)
                assert loss.item() == pytest.approx(MR.per_sample(pred, target, q).mean().item(), rel=1e-13)


@pytest.mark.parametrize("bg", [0.0, 0.1, 0.25, 1.0])
def test_all_foreground_is_exactly_one_and_empty_is_zero(bg):
    full = torch.full((24, 40), 255, dtype=torch.uint8)
    assert bool((MR.weights_from_mask(full, 8, 3, bg).float() == 1.0).all())
    assert bool((MR.weights_from_mask(torch.full((24, 40), 3, dtype=torch.uint8), 8, 3, bg).float() == 1.0).all())
    empty = MR.weights_from_mask(torch.full((24, 40), 2, dtype=torch.uint8), 8, 3, bg)
    if bg == 0.0:
        assert bool((empty == 0.0).all()) and bool(torch.isfinite(empty).all())
    else:  # a uniform background weight is the plain loss
        assert bool((empty.float() == 1.0).all())
    ones = torch.ones(2, 15, dtype=torch.float64)
    p, t = torch.randn(2, 4, 15, dtype=torch.float64), torch.randn(2, 4, 15, dtype=torch.float64)
    assert MR.weighted_loss(p, t, ones)[0].item() == pytest.approx(((p - t) ** 2).mean().item(), rel=1e-14)


# ------------------------------------------------------------------------------------------------ the plan's geometry
def test_geometric_plan_keeps_rotate_and_rrcrop_only():
    plan = [("jitter", [0, 1, 2, 3], 1.0, 1.0, 1.0, 0.0), ("gray",), ("blur", 0.15), ("rotate", 3.5),
            ("rrcrop", 1, 2, 30, 40, 64, 64)]
    assert A.geometric_plan(plan) == [("rotate", 3.5), ("rrcrop", 1, 2, 30, 40, 64, 64)]
    assert A.geometric_plan([]) == [] and A.geometric_plan(plan[:3]) == []
    seen = set()
    for key in range(1, 9):  # every pipeline: the geometric part is the plan's sub-sequence, in order
        for seed in range(4):
            torch.manual_seed(seed)
            p = A.draw_plan(key, (64, 64), 64, 64)
            gp = A.geometric_plan(p)
            assert gp == [op for op in p if op[0] in ("rotate", "rrcrop")]
            seen.update(op[0] for op in p)
    assert {"jitter", "blur", "rotate", "rrcrop"} <= seen  # (gray has p = 0.1: these few draws need not hit it)
    # a rotation brings background in: fill 0 at the corners of an all-foreground mask
    full = Image.fromarray(np.full((48, 64, 3), 255, dtype=np.uint8))
    r = np.asarray(A.apply_plan(full, [("rotate", 10.0)], fill=0))
    assert r[0, 0, 0] == 0 and r[-1, -1, 0] == 0 and r[24, 32, 0] == 255


# ------------------------------------------------------------------------------------------------ the data set
def _toys(root, n=3, size=64):
    img, msk = root / "img", root / "msk"
    img.mkdir(parents=True)
    msk.mkdir(parents=True)
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 255, (size, size, 3), dtype=np.uint8)).save(img / f"{i}.png")
        m = np.zeros((size, size), dtype=np.uint8)
        m[:, : size // 2] = 255  # the left half-plane is the object
        Image.fromarray(m).save(msk / f"{i}.png")
    return img, msk


def _dataset(img, tk=None, **kw):
    if tk is None:
        tk = HashTokenizer()
        tk.add_tokens(["<toy>"])
    return TextualInversionDataset(img, tk, learnable_mode=0, size=64, placeholder_object_token="<toy>", **kw)


@pytest.mark.parametrize("key", [0, 1, 5, 7])
def test_images_and_generator_are_those_of_a_run_without_masks(tmp_path, key):
    import random
    img, msk = _toys(tmp_path)
    plain, masked = _dataset(img, augmentation_key=key, flip_p=0.5), _dataset(img, augmentation_key=key, flip_p=0.5, mask_dir=msk)
    for seed in range(4):
        outs = []
        for ds in (plain, masked):
            torch.manual_seed(seed)
            random.seed(seed)
            ex = [ds[i] for i in range(3)]
            outs.append((ex, torch.get_rng_state(), random.getstate()))
        (a, ra, pa), (b, rb, pb) = outs
        assert torch.equal(ra, rb) and pa == pb, "the option changed what the sample draws"
        for x, y in zip(a, b):
            assert torch.equal(x["pixel_values"], y["pixel_values"]) and torch.equal(x["input_ids"], y["input_ids"])
            assert "loss_mask" not in x and y["loss_mask"].dtype == torch.uint8 and tuple(y["loss_mask"].shape) == (64, 64)
    batch = TextualInversionDataset.collate([masked[0], masked[1]])
    assert batch["loss_mask"].dtype == torch.uint8 and tuple(batch["loss_mask"].shape) == (2, 64, 64)


def test_device_pipeline_samples_name_the_mask(tmp_path):
    img, msk = _toys(tmp_path)
    for seed in range(3):
        plans = []
        for kw in ({}, {"mask_dir": msk}):
            torch.manual_seed(seed)
            plans.append(_dataset(img, augmentation_key=1, device_pipeline=True, **kw)[1]["aug"])
        assert {k: v for k, v in plans[1].items() if k != "mask_path"} == plans[0]
        assert plans[1]["mask_path"] == str(msk / "1.png") and "mask_path" not in plans[0]


def test_mask_follows_the_flip_and_the_crop(tmp_path):
    img, msk = _toys(tmp_path)
    ds = _dataset(img, mask_dir=msk)
    path = ds.image_paths[0]
    m = ds.load_mask(path)
    assert m.dtype == np.uint8 and m.shape == (64, 64) and (m[:, :32] == 255).all() and (m[:, 32:] == 0).all()
    f = ds.load_mask(path, flip=True)
    assert (f[:, :32] == 0).all() and (f[:, 32:] == 255).all()
    # crop rows 0..31, columns 16..47 (the edge at column 32 is the crop's column 16 of 32), back up to 64 x 64: the edge
    # lands at column 32 again, with at most the bilinear filter's two grey columns either side
    c = ds.load_mask(path, plan=[("jitter", [0, 1, 2, 3], 0.9, 1.1, 1.0, 0.01), ("blur", 0.15),
                                 ("rrcrop", 0, 16, 32, 32, 64, 64)])
    assert (c[:, :30] == 255).all() and (c[:, 34:] == 0).all()
    # crop columns 0..31 only: all object; columns 32..63 only: none
    assert (ds.load_mask(path, plan=[("rrcrop", 8, 0, 32, 32, 64, 64)]) == 255).all()
    assert (ds.load_mask(path, plan=[("rrcrop", 8, 32, 32, 32, 64, 64)]) == 0).all()
    # flipped, then cropped to what was the left half: none
    assert (ds.load_mask(path, flip=True, plan=[("rrcrop", 0, 0, 64, 32, 64, 64)]) == 0).all()
    # through __getitem__ with flip_p = 1: the sample's mask is the flipped one
    torch.manual_seed(0)
    ex = _dataset(img, mask_dir=msk, flip_p=1.0)[0]
    assert torch.equal(ex["loss_mask"], torch.from_numpy(f))
    # and the weights: 4 of 8 cell columns carry the whole loss
    q = MR.weights_from_mask(ex["loss_mask"], 8).view(8, 8)
    assert bool((q[:, :4] == 0).all()) and bool((q[:, 4:] == 2.0).all())


def test_a_missing_or_misfit_mask_raises_at_construction(tmp_path):
    img, msk = _toys(tmp_path)
    (msk / "1.png").unlink()
    with pytest.raises(FileNotFoundError, match="1.png"):
        _dataset(img, mask_dir=msk)
    Image.fromarray(np.zeros((32, 32), dtype=np.uint8)).save(msk / "1.png")
    with pytest.raises(ValueError, match="pixel grid"):
        _dataset(img, mask_dir=msk)


def test_dtu_lookup_is_that_of_get_object_masks(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cal = tmp_path / "data" / "dtu" / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    rng = np.random.RandomState(1)
    for i in range(49):
        np.savetxt(cal / f"pos_{i + 1:03d}.txt", rng.randn(3, 4))
    root = tmp_path / "data" / "dtu" / "Rectified"
    for scan in ("scan8", "scan21"):
        (root / scan).mkdir(parents=True)
        for c in range(49):
            Image.fromarray(rng.randint(0, 255, (30, 40, 3), dtype=np.uint8)).save(
                root / scan / TextualInversionDataset.dtu_cam_and_lighting_to_fname(c, "3"))
    masks = tmp_path / "idr"
    for scan, sub in (("scan8", "mask"), ("scan21", "")):  # both layouts of inference_dtu.py:375-398
        d = masks / scan / sub
        d.mkdir(parents=True)
        for c in range(49):
            Image.fromarray(np.full((30, 40), 255 if scan == "scan8" else 0, dtype=np.uint8)).save(d / f"{c:03d}.png")
    tk = HashTokenizer()
    kw = dict(camera_representation="dtu-12d", dtu_subset=3, dtu_lighting=3, dtu_preprocess_key=1)
    ds = TextualInversionDataset(root / "scan8", tk, learnable_mode=2, placeholder_object_token="<object>", mask_dir=masks, **kw)
    assert [ds.mask_path(p) for p in ds.image_paths] == [masks / "scan8" / "mask" / f"{c:03d}.png" for c in (22, 25, 28)]
    from view_neti_amd.compat.dtu_metrics import get_object_masks
    assert np.array_equal(np.asarray(get_object_masks([22], 8, 0, masks)[22])[..., 0], np.asarray(Image.open(ds.mask_path(ds.image_paths[0]))))
    # mode 3: the scan of the object being sampled
    np.random.seed(0)
    ds3 = TextualInversionDataset(root, tk, learnable_mode=3, train_data_subsets=["scan8", "scan21"],
                                  placeholder_object_tokens=["<scan8>", "<scan21>"], mask_dir=masks, **kw)
    tk.add_tokens(ds3.placeholder_tokens)
    for k, (scan, value) in enumerate((("scan8", 255), ("scan21", 0))):
        ds3.current_object_idx = k
        ex = ds3[0]
        assert scan in ex["text"] and tuple(ex["loss_mask"].shape) == (384, 512) and bool((ex["loss_mask"] == value).all())
    (masks / "scan21" / "025.png").unlink()
    with pytest.raises(FileNotFoundError, match="025.png"):
        TextualInversionDataset(root, tk, learnable_mode=3, train_data_subsets=["scan8", "scan21"],
                                placeholder_object_tokens=["<scan8>", "<scan21>"], mask_dir=masks, **kw)


# ------------------------------------------------------------------------------------------------ configuration
def test_fields_parse_and_validate(tmp_path):
    cfg = C.parse(C.RunConfig, ["--data.mask_dir", str(tmp_path), "--optim.loss_mask_background", "0.25",
                                "--eval.heldout_loss_masked", "true"])
    assert cfg.data.mask_dir == tmp_path and cfg.optim.loss_mask_background == 0.25 and cfg.eval.heldout_loss_masked is True
    plain = C.parse(C.RunConfig, [])
    assert plain.data.mask_dir is None and plain.optim.loss_mask_background == 0.0 and plain.eval.heldout_loss_masked is False
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="loss_mask_background"):
            C.parse(C.RunConfig, ["--data.mask_dir", str(tmp_path), "--optim.loss_mask_background", bad])
    for ok in ("0", "1"):
        C.parse(C.RunConfig, ["--data.mask_dir", str(tmp_path), "--optim.loss_mask_background", ok])
    with pytest.raises(ValueError, match="mask_dir"):
        C.parse(C.RunConfig, ["--optim.loss_mask_background", "0.25"])
    with pytest.raises(ValueError, match="mask_dir"):
        C.parse(C.RunConfig, ["--eval.heldout_loss_masked", "true"])
    again = C.decode(C.RunConfig, __import__("yaml").safe_load(C.dump(cfg)))
    assert again.data.mask_dir == tmp_path and again.optim.loss_mask_background == 0.25


def test_what_a_checkpoint_and_config_yaml_carry(tmp_path):
    cfg = C.parse(C.RunConfig, ["--data.mask_dir", str(tmp_path), "--optim.loss_mask_background", "0.25"])
    ckpt_cfg = C.encode(cfg, include_ext=False)
    assert "mask_dir" not in ckpt_cfg["data"] and "loss_mask_background" not in ckpt_cfg["optim"]
    C.decode(C.RunConfig, ckpt_cfg)  # still the reference's schema
    ext = C.ext_fields(cfg)
    assert ext["data.mask_dir"] == tmp_path and ext["optim.loss_mask_background"] == 0.25
    only = C.parse(C.RunConfig, ["--data.mask_dir", str(tmp_path)])
    assert "optim.loss_mask_background" not in C.ext_fields(only) and "loss_mask_background" not in C.encode(only)["optim"]
    assert "heldout_loss_masked" not in C.encode(only)["eval"]
    plain = C.parse(C.RunConfig, [])  # a run without the option writes the files it always wrote
    assert not any("mask" in k for k in C.ext_fields(plain))
    enc = C.encode(plain)
    assert "mask_dir" not in enc["data"] and "loss_mask_background" not in enc["optim"] and "heldout_loss_masked" not in enc["eval"]


def test_fingerprint_and_trainer_state_refusal():
    args = (0, 2, 2, 1, "fp16", 0, 300, 1234)
    unset = R.fingerprint(*args)
    on, on_bg = R.fingerprint(*args, loss_mask=True), R.fingerprint(*args, loss_mask=True, loss_mask_background=0.25)
    assert "loss_mask" not in unset and "loss_mask_background" not in unset
    assert on["loss_mask"] is True and "loss_mask_background" not in on and on_bg["loss_mask_background"] == 0.25
    assert {k: v for k, v in on_bg.items() if not k.startswith("loss_mask")} == unset
    assert unset == {k: v for k, v in R.fingerprint(*args, snr_gamma=5.0).items() if k != "snr_gamma"}
    for fp in (unset, on, on_bg):
        R.check_fingerprint(fp, fp)
    # a state saved with the option is refused without it, and the reverse; another background weight too
    for saved, current, field in ((on, unset, "loss_mask"), (unset, on, "loss_mask"), (on_bg, on, "loss_mask_background"),
                                  (on, on_bg, "loss_mask_background"),
                                  (on_bg, R.fingerprint(*args, loss_mask=True, loss_mask_background=0.5), "loss_mask_background")):
        with pytest.raises(ValueError, match=field) as err:
            R.check_fingerprint(saved, current)
        assert "learnable_mode" not in str(err.value)
    from view_neti_amd.engine.step import TrainStepEngine
    assert "loss_mask" in TrainStepEngine._WHEN_SET and "loss_mask_background" in TrainStepEngine._WHEN_SET
    assert "loss_weights" not in TrainStepEngine._STATE  # the table is rewritten for every batch: not state


# ------------------------------------------------------------------------------------------------ train-metrics.jsonl
def test_masked_mark_only_when_set():
    closed = {"skipped": False, "clip_coef": 1.0, "loss_scale": 65536.0, "lr": 0.5,
              "grad_norm": {"object": 3.0, "view": 4.0, "total": 5.0}}
    group = [{"micro_step": 0, "micro": 0, "closed": True, "timesteps": [0, 146], "losses": [0.5, 0.25], **closed}]
    plain = TM.step_line(3, group)
    assert "masked" not in plain
    line = TM.step_line(3, group, masked=True)
    assert line["masked"] is True and {k: v for k, v in line.items() if k != "masked"} == plain
    assert json.loads(json.dumps(line, allow_nan=False)) == line
    assert TM.lines_up_to([group], 3, masked=True)[0]["masked"] is True


def test_heldout_record_carries_loss_masked():
    from view_neti_amd.compat import heldout as HL
    p = HL.plan(2, "dtu-12d", 3, ["<object>"], 2, 3)
    rows = [(it, 1.0 + it.cam + 0.25 * it.k) for items, n in p.batches["<object>"] for it in items[:n]]
    mrows = [(it, 0.5 * v) for it, v in rows]
    plain = HL.make_record(7, p, {"<object>": rows})
    rec = HL.make_record(7, p, {"<object>": rows}, masked_losses={"<object>": mrows})
    o = rec["objects"]["<object>"]
    assert {k: v for k, v in o.items() if k != "loss_masked"} == plain["objects"]["<object>"]
    m = o["loss_masked"]
    assert m["train"] == pytest.approx(0.5 * o["train"]) and m["test"] == pytest.approx(0.5 * o["test"])
    for it, v in mrows:  # one value per (camera, timestep)
        assert m["by_view_timestep"][str(it.cam)][str(it.timestep)] == v
    assert "loss_masked" not in plain["objects"]["<object>"]
