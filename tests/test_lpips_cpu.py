"""CPU: LPIPS-VGG around the GPU engine — the weight loaders (torchvision / lpips key names and shapes), the host
restatement (tests/helpers/lpips_ref.py) against a hand-written per-pixel evaluation, the InferenceConfig switches, and
summarize_dtu on synthetic run directories with the restatement injected."""
import csv

import numpy as np
import pytest
import torch

from helpers import lpips_ref


def test_loaders_accept_reference_keys_and_reject_bad_ones(tmp_path):
    from view_neti_amd.compat import lpips as L
    vgg, lin = lpips_ref.synthetic_weights(0)
    full = dict(vgg, **{"classifier.0.weight": torch.zeros(4, 4)})  # torchvision's file also holds the classifier
    torch.save(full, tmp_path / "vgg16-397923af.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    v = L.load_vgg16_features(tmp_path / "vgg16-397923af.pth")
    l = L.load_lpips_lin(tmp_path / "vgg.pth")
    assert set(v) == set(vgg) and set(l) == set(lin) and torch.equal(v["features.28.weight"], vgg["features.28.weight"])
    bad = dict(vgg)
    del bad["features.17.bias"]
    with pytest.raises(KeyError, match="features.17.bias"):
        L.load_vgg16_features(bad)
    bad = dict(vgg, **{"features.5.weight": torch.zeros(128, 64, 1, 1)})
    with pytest.raises(ValueError, match="features.5.weight"):
        L.load_vgg16_features(bad)
    bad = dict(lin, **{"lin3.model.1.weight": torch.zeros(1, 256, 1, 1)})
    with pytest.raises(ValueError, match="lin3.model.1.weight"):
        L.load_lpips_lin(bad)
    with pytest.raises(FileNotFoundError):
        L.LPIPS.from_files(tmp_path / "missing.pth", tmp_path / "vgg.pth")


def _hand_lpips_two_stages(x0, x1, vgg, lin):
    """the algorithm pixel by pixel in float64 numpy: scaling, zero-padded 3x3 convolutions, ReLU, 2x2 pool, and the
    normalised weighted distance of relu1_2 and relu2_2"""
    shift = np.array([-.030, -.088, -.188]).reshape(3, 1, 1)
    scale = np.array([.458, .448, .450]).reshape(3, 1, 1)

    def conv_relu(h, i):
        w = vgg[f"features.{i}.weight"].double().numpy()
        b = vgg[f"features.{i}.bias"].double().numpy()
        C, H, W = h.shape
        p = np.pad(h, ((0, 0), (1, 1), (1, 1)))
        out = np.empty((w.shape[0], H, W))
        for y in range(H):
            for x in range(W):
                out[:, y, x] = np.einsum("ocij,cij->o", w, p[:, y:y + 3, x:x + 3]) + b
        return np.maximum(out, 0)

    def pool(h):
        C, H, W = h.shape
        return h[:, :H // 2 * 2, :W // 2 * 2].reshape(C, H // 2, 2, W // 2, 2).max(axis=(2, 4))

    def taps(img):
        h = (img.double().numpy() - shift) / scale
        t1 = conv_relu(conv_relu(h, 0), 2)
        t2 = conv_relu(conv_relu(pool(t1), 5), 7)
        return [t1, t2]

    total = 0.0
    for k, (a, b) in enumerate(zip(taps(x0), taps(x1))):
        w = lin[f"lin{k}.model.1.weight"].double().numpy().reshape(-1)
        C, H, W = a.shape
        acc = 0.0
        for y in range(H):
            for x in range(W):
                na = a[:, y, x] / (np.sqrt((a[:, y, x] ** 2).sum()) + 1e-10)
                nb = b[:, y, x] / (np.sqrt((b[:, y, x] ** 2).sum()) + 1e-10)
                acc += float((w * (na - nb) ** 2).sum())
        total += acc / (H * W)
    return total


def test_oracle_identity_symmetry_and_hand_evaluation():
    vgg, lin = lpips_ref.synthetic_weights(1)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 12, 16, generator=g) * 2 - 1
    y = torch.rand(2, 3, 12, 16, generator=g) * 2 - 1
    assert torch.equal(lpips_ref.lpips(x, x, vgg, lin, n_stages=2), torch.zeros(2, 1, 1, 1))
    d = lpips_ref.lpips(x, y, vgg, lin, n_stages=2)
    assert d.shape == (2, 1, 1, 1) and (d > 0).all()
    assert torch.allclose(d, lpips_ref.lpips(y, x, vgg, lin, n_stages=2), rtol=1e-6, atol=0)
    for b in range(2):
        ref = _hand_lpips_two_stages(x[b], y[b], vgg, lin)
        assert abs(d[b].item() - ref) <= 1e-5 * ref


def test_inference_config_lpips_switches(tmp_path):
    from view_neti_amd.compat.inference_dtu import InferenceConfig, parse_inference_config
    c = InferenceConfig()
    assert c.do_lpips is False and c.lpips_vgg_weights is None and c.lpips_lin_weights is None
    with pytest.raises(ValueError, match="lpips"):
        InferenceConfig(do_lpips=True)
    with pytest.raises(ValueError, match="lpips"):
        InferenceConfig(do_lpips=True, lpips_vgg_weights="a", lpips_lin_weights="b", torch_dtype="bf16")
    c = parse_inference_config(["--input_dir", str(tmp_path), "--iteration", "1500", "--do_lpips", "true",
                                "--lpips_vgg_weights", "A.pth", "--lpips_lin_weights", "B.pth"])
    assert c.do_lpips is True and str(c.lpips_vgg_weights) == "A.pth" and str(c.lpips_lin_weights) == "B.pth"


def _write_run(run, subset, it, result, keyed):
    from view_neti_amd.compat import config as cfgmod
    run.mkdir(parents=True)
    cfg = cfgmod.RunConfig()
    cfg.data.dtu_subset = subset
    torch.save({"cfg": cfgmod.encode(cfg, include_ext=False)}, run / f"mapper-steps-{it}_view.pt")
    (run / "inference").mkdir()
    torch.save({None: result} if keyed else result, run / "inference" / f"results_all_iter_{it}_scans_[None]_seeds_[0, 1].pt")


def _result(seed, V=3, H=16, W=20):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(V, 3, H, W, generator=g)
    masks = torch.zeros(V, 3, H, W)
    masks[:, :, 2:14, 3:18] = 1.0
    preds = [(gt + 0.1 * torch.randn(V, 3, H, W, generator=g)).clamp(0, 1) for _ in range(2)]
    return dict(imgs_gt=gt, masks=masks, imgs_pred=preds)


def test_summarize_dtu_rows(tmp_path):
    from view_neti_amd.compat import dtu_metrics as dm
    from view_neti_amd.compat.summarize_dtu import main
    vgg, lin = lpips_ref.synthetic_weights(2)
    oracle = lpips_ref.Oracle(vgg, lin)
    res = {"a": _result(10), "b": _result(11), "c": _result(12)}
    _write_run(tmp_path / "scan1_subs_1", 1, 1500, res["a"], keyed=True)
    _write_run(tmp_path / "scan2_subs_1", 1, 1500, res["b"], keyed=False)
    _write_run(tmp_path / "scan1_subs_3", 3, 1500, res["c"], keyed=True)
    out = tmp_path / "summary.csv"
    main(["--runs", str(tmp_path / "scan*_subs_*"), "--iterations", "1500", "--out", str(out)], lpips_fn=oracle)

    def per_seed(r):
        m, gt = r["masks"], r["imgs_gt"] * r["masks"]
        rows = []
        for p in r["imgs_pred"]:
            pm = p * m
            lp = oracle(pm * 2 - 1, gt * 2 - 1)[:, 0, 0, 0].mean().item()
            ss = dm.ssim_fn_batch(pm, gt).mean().item()
            mse = ((gt - pm) ** 2).reshape(3, -1).sum(-1) / m.reshape(3, -1).sum(-1)
            rows.append((lp, ss, dm.mse_to_psnr(mse).mean().item()))
        return np.array(rows)

    expect = {1: (per_seed(res["a"]) + per_seed(res["b"])) / 2, 3: per_seed(res["c"])}
    with open(out) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == ["num_imgs", "dtu_subset", "iteration", "seed", "lpips", "ssim", "psnr"]
    assert [(r["num_imgs"], r["dtu_subset"], r["iteration"], r["seed"]) for r in rows] == \
        [("1", "1", "1500", "0"), ("1", "1", "1500", "1"), ("3", "3", "1500", "0"), ("3", "3", "1500", "1")]
    for r in rows:
        e = expect[int(r["dtu_subset"])][int(r["seed"])]
        got = np.array([float(r["lpips"]), float(r["ssim"]), float(r["psnr"])])
        assert np.allclose(got, e, rtol=1e-5, atol=0), (got, e)
    assert all(float(r["lpips"]) > 0 for r in rows)
