"""Held-out validation, the parts that need no GPU: the evaluation plan (timesteps, seeds, packing, splits),
the fixed noise, the configuration keys and the jsonl record."""
import json

import pytest
import torch

from view_neti_amd.compat import config as C
from view_neti_amd.compat import heldout as H
from view_neti_amd.compat.dtu_metrics import get_cam_idxs


def test_timesteps_are_slice_midpoints():
    assert H.eval_timesteps(1) == [500]
    assert H.eval_timesteps(4) == [125, 375, 625, 875]
    assert H.eval_timesteps(7) == [71, 214, 357, 500, 642, 785, 928]
    for K in (1, 4, 7):
        assert H.eval_timesteps(K) == [((2 * k + 1) * 1000) // (2 * K) for k in range(K)]
    with pytest.raises(ValueError):
        H.eval_timesteps(0)


def test_noise_seed_and_draw_order():
    assert H.noise_seed(0, 0, 0) == 0 and H.noise_seed(7, 22, 3) == 7 + 22000 + 3
    eps, noise = H.fixed_noise(7, 22, 3, 6, 8)
    g = torch.Generator().manual_seed(22010)
    assert torch.equal(eps, torch.randn((4, 6, 8), generator=g)), "eps is the generator's first draw"
    assert torch.equal(noise, torch.randn((4, 6, 8), generator=g)), "noise is its second"
    assert not torch.equal(eps, noise)


@pytest.mark.parametrize("subset", [1, 3, 6, 9, 0])
def test_plan_splits_follow_get_cam_idxs(subset):
    cams, train, test = get_cam_idxs(subset)
    p = H.plan(2, "dtu-12d", subset, ["<object>"], 4, 4)
    assert p.cams == cams and len(cams) == 34
    assert p.cams_train == train and p.cams_test == test
    items = [it for entries, n in p.batches["<object>"] for it in entries[:n]]
    assert len(items) == 34 * 4 == p.n_items("<object>")
    assert {it.cam for it in items if it.split == "train"} == set(train) & set(cams)
    assert {it.cam for it in items if it.split == "test"} == set(test)
    assert all(it.timestep == p.timesteps[it.k] for it in items)
    # object x camera x k, in that nesting order
    assert [(it.cam, it.k) for it in items] == [(c, k) for c in cams for k in range(4)]


def test_plan_packs_with_a_padded_last_batch():
    p = H.plan(2, "dtu-12d", 3, ["<object>"], 4, 3)  # 136 items in batches of 3: 45 full ones and one real item
    batches = p.batches["<object>"]
    assert len(batches) == 46 and all(len(e) == 3 for e, _ in batches)
    assert [n for _, n in batches] == [3] * 45 + [1]
    last, n = batches[-1]
    assert last[1] == last[0] and last[2] == last[0], "the partial batch repeats its last real entry"
    # one batch, more room than items
    q = H.plan(2, "dtu-12d", 3, ["<object>"], 1, 64)
    (entries, n), = q.batches["<object>"]
    assert n == 34 and len(entries) == 64 and all(e == entries[33] for e in entries[34:])


def test_plan_mode0_and_mode3_forms():
    p0 = H.plan(0, "spherical", -2, ["<toy>"], 2, 4, n_train_images=5)
    assert p0.cams == [0, 1, 2, 3, 4] and p0.cams_train == p0.cams and p0.cams_test == []
    assert all(it.split == "train" for e, n in p0.batches["<toy>"] for it in e)
    assert p0.n_items("<toy>") == 10
    with pytest.raises(ValueError):
        H.plan(0, "spherical", -2, ["<toy>"], 2, 4, n_train_images=0)
    p3 = H.plan(3, "dtu-12d", 3, ["<scan65>", "<scan125>"], 2, 4)
    assert list(p3.batches) == ["<scan65>", "<scan125>"]
    for tok in p3.batches:  # packed per object: no batch mixes two objects
        assert all(it.obj == tok for e, n in p3.batches[tok] for it in e)
        assert p3.n_items(tok) == 34 * 2
    with pytest.raises(NotImplementedError):
        H.plan(2, "spherical", 3, ["<object>"], 4, 4)


def test_noise_of_an_item_does_not_depend_on_the_batch_size():
    def by_item(batch):
        p = H.plan(2, "dtu-12d", 3, ["<object>"], 3, batch)
        out = {}
        for entries, n in p.batches["<object>"]:
            eps = torch.stack([H.fixed_noise(5, it.cam, it.k, 4, 6)[0] for it in entries])
            noise = torch.stack([H.fixed_noise(5, it.cam, it.k, 4, 6)[1] for it in entries])
            for i, it in enumerate(entries[:n]):
                out[(it.cam, it.k)] = (eps[i], noise[i])
        return out
    a, b = by_item(1), by_item(7)
    assert a.keys() == b.keys() and len(a) == 34 * 3
    assert all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)
    assert not torch.equal(a[(22, 0)][0], a[(22, 1)][0]) and not torch.equal(a[(22, 0)][0], a[(23, 0)][0])


def test_config_keys_parse_and_stay_out_of_checkpoints(tmp_path):
    d = C.parse(C.RunConfig, [])
    assert (d.eval.heldout_loss_steps, d.eval.heldout_loss_timesteps, d.eval.heldout_loss_seed) == (0, 4, 0)
    assert d.eval.validation_nvs is False and d.eval.validation_nvs_batch == 4
    assert d.eval.lpips_vgg_weights is None and d.eval.lpips_lin_weights is None
    # defaults leave config.yaml as it always was
    assert not {"heldout_loss_steps", "validation_nvs", "lpips_vgg_weights"} & set(C.encode(d)["eval"])
    cli = C.parse(C.RunConfig, ["--eval.heldout_loss_steps", "250", "--eval.heldout_loss_timesteps", "7",
                                "--eval.heldout_loss_seed", "11", "--eval.validation_nvs", "True",
                                "--eval.validation_nvs_batch", "2", "--eval.lpips_vgg_weights", "vgg.pth"])
    y = tmp_path / "c.yaml"
    y.write_text("eval: {heldout_loss_steps: 250, heldout_loss_timesteps: 7, heldout_loss_seed: 11, validation_nvs: true,\n"
                 "       validation_nvs_batch: 2, lpips_vgg_weights: vgg.pth}\n")
    for cfg in (cli, C.parse(C.RunConfig, ["--config_path", str(y)])):
        e = cfg.eval
        assert (e.heldout_loss_steps, e.heldout_loss_timesteps, e.heldout_loss_seed) == (250, 7, 11)
        assert e.validation_nvs is True and e.validation_nvs_batch == 2 and str(e.lpips_vgg_weights) == "vgg.pth"
        # config.yaml names them where they are set; a checkpoint's cfg and its extension record never do
        assert C.encode(cfg)["eval"]["heldout_loss_steps"] == 250
        ckpt_cfg = C.encode(cfg, include_ext=False)
        new = {"heldout_loss_steps", "heldout_loss_timesteps", "heldout_loss_seed", "validation_nvs",
               "validation_nvs_batch", "lpips_vgg_weights", "lpips_lin_weights"}
        assert not new & set(ckpt_cfg["eval"])
        assert not any(k.split(".")[-1] in new for k in C.ext_fields(cfg))
        C.decode(C.RunConfig, ckpt_cfg)  # and that cfg still decodes
    with pytest.raises(ValueError):
        C.parse(C.RunConfig, ["--eval.heldout_loss_timesteps", "0"])


def test_jsonl_record_round_trips(tmp_path):
    p = H.plan(2, "dtu-12d", 3, ["<object>"], 2, 4)
    rows = [(it, 0.5 + 0.001 * it.cam + 0.1 * it.k) for e, n in p.batches["<object>"] for it in e[:n]]
    rec = H.make_record(250, p, {"<object>": rows})
    assert rec["step"] == 250 and rec["timesteps"] == [250, 750] and list(rec["objects"]) == ["<object>"]
    o = rec["objects"]["<object>"]
    tr = [v for it, v in rows if it.split == "train"]
    te = [v for it, v in rows if it.split == "test"]
    assert len(tr) == 3 * 2 and len(te) == 31 * 2
    assert o["train"] == pytest.approx(sum(tr) / len(tr)) and o["test"] == pytest.approx(sum(te) / len(te))
    assert set(o["by_timestep"]) == {"250", "750"} and set(o["by_view"]) == {str(c) for c in p.cams}
    assert o["by_view"]["22"] == pytest.approx(0.5 + 0.022 + 0.05)
    assert o["by_timestep"]["750"]["test"] == pytest.approx(sum(v for it, v in rows if it.split == "test" and it.k == 1) / 31)
    f = tmp_path / H.FILE_NAME
    H.append_record(f, rec)
    H.append_record(f, H.make_record(500, p, {"<object>": rows}))
    lines = f.read_text().splitlines()
    assert len(lines) == 2 and json.loads(lines[0]) == rec
    back = H.read_records(f)
    assert [r["step"] for r in back] == [250, 500]
    assert back[0]["objects"]["<object>"]["by_view"][22] == o["by_view"]["22"]
    assert back[0]["objects"]["<object>"]["by_timestep"][250] == o["by_timestep"]["250"]
    # an empty split (mode 0 has no test cameras) is null, not a division by zero
    p0 = H.plan(0, "spherical", 0, ["<toy>"], 1, 2, n_train_images=2)
    r0 = H.make_record(1, p0, {"<toy>": [(it, 1.0) for e, n in p0.batches["<toy>"] for it in e[:n]]})
    assert r0["objects"]["<toy>"]["test"] is None and r0["objects"]["<toy>"]["train"] == 1.0
    assert "n/a" in H.summary_line(1, r0) and "n/a" in H.format_table([r0])
