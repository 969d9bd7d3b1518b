"""LPIPS-VGG on the GPU (csrc/lpips.hip, engine/lpips.py, compat/lpips.py): the glue kernels bit-exact or within 1e-5 of
torch, the whole metric against the fp32 host restatement (tests/helpers/lpips_ref.py) at 60x84 and the 300x400 DTU
evaluation size, its exact properties (identity, symmetry, reproducibility, position and sub-batch independence), and the
DTU harness with do_lpips on a synthetic scene."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import lpips_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.fixture(scope="module")
def weights():
    return lpips_ref.synthetic_weights(0)


def _images(B, H, W, seed):
    """smooth random images in [-1, 1]: half of them masked copies of the other half (a centred box kept)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(2, H // 8), max(2, W // 8), generator=g)
    img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    img = (img + 0.05 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    return img * 2 - 1


def test_relu_maxpool_odd_extents():
    from view_neti_amd import ops
    g = torch.Generator().manual_seed(0)
    for (H, W, C) in ((75, 100, 256), (37, 50, 512)):
        x = (torch.randn(2, H, W, C, generator=g)).half().to(DEV)
        y = torch.empty(2, H // 2, W // 2, C, dtype=torch.float16, device=DEV)
        ops.relu_maxpool2x2(x, y, 2, H, W, C)
        ref = F.relu(F.max_pool2d(x.permute(0, 3, 1, 2).float(), 2)).half().permute(0, 2, 3, 1)
        assert y.shape == ref.shape and torch.equal(y, ref)
    z = torch.randn(4096, generator=g).half().to(DEV)
    r = F.relu(z.float()).half()
    ops.relu_(z)
    assert torch.equal(z, r)


def test_prep_is_scaled_im2col_with_zero_border():
    from view_neti_amd import ops
    g = torch.Generator().manual_seed(1)
    B, H, W = 2, 30, 41
    nhwc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    x = nhwc.permute(0, 3, 1, 2).to(DEV)  # non-contiguous NCHW view
    out = torch.full((B * H * W, 64), 7.0, dtype=torch.float16, device=DEV)
    ops.lpips_prep(x, out, B, H, W)
    scaled = lpips_ref.scaling_layer(x.cpu())
    unf = F.unfold(F.pad(scaled, (1, 1, 1, 1)), 3)  # [B, c*9 + tap, L]
    ref = unf.view(B, 3, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 27).half()
    got = out.cpu()
    assert torch.equal(got[:, :27], ref) and (got[:, 27:] == 0).all()
    # the top-left pixel's upper-left tap is the zero border, not (0 - shift) / scale
    assert (got[0, :3] == 0).all()


@pytest.mark.parametrize("C,HW", [(64, 60 * 84), (128, 30 * 42), (256, 75 * 100), (512, 37 * 50), (512, 18 * 25)])
def test_layer_distance_matches_f32_torch(C, HW):
    from view_neti_amd import ops
    g = torch.Generator().manual_seed(C + HW)
    n = 4
    feat = (torch.randn(n, HW, C, generator=g) * 2).half()
    w = torch.rand(C, generator=g) / C
    pairs = torch.tensor([[1, 0], [2, 0], [3, 0], [0, 3], [2, 2]], dtype=torch.int32)  # ground truth 0 reused
    f = F.relu(feat.float())
    nrm = f / (f.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    ref = torch.stack([((nrm[i] - nrm[j]) ** 2 * w).sum(-1).mean() for i, j in pairs.tolist()])
    ws = torch.empty(ops.lpips_ws_floats(len(pairs), C, HW), device=DEV)
    out = torch.empty(len(pairs), device=DEV)
    fd, pd, wd = feat.to(DEV), pairs.to(DEV), w.to(DEV)
    ops.lpips_distance(fd, n, pd, wd, C, HW, ws, out)
    got = out.cpu()
    assert got[4] == 0
    assert ((got[:4] - ref[:4]).abs() <= 1e-5 * ref[:4].abs()).all(), (got, ref)
    ops.lpips_distance(fd, n, pd, wd, C, HW, ws, out, accumulate=True)
    assert torch.equal(out.cpu(), got + got)


@pytest.mark.parametrize("H,W,B", [(60, 84, 6), (300, 400, 2)])
def test_whole_metric_against_oracle(weights, H, W, B):
    from view_neti_amd.engine.lpips import LPIPSEngine
    vgg, lin = weights
    eng = LPIPSEngine(vgg, lin, H, W, max_images=2 * B, device=DEV)
    base = _images(B, H, W, seed=H)
    other = _images(B, H, W, seed=H + 1)
    mask = torch.zeros(1, 1, H, W)
    mask[..., H // 5:4 * H // 5, W // 6:5 * W // 6] = 1
    in0 = base.clone()
    in1 = torch.where(torch.arange(B).view(B, 1, 1, 1) % 2 == 0, (base + 1) * mask - 1, other)  # masked copy | unrelated
    got = eng(in0, in1).cpu()
    ref = lpips_ref.lpips(in0, in1, vgg, lin)
    err = (got - ref).abs()
    print(f"LPIPS {H}x{W}: max |delta| {err.max().item():.3e}, max rel {(err / ref.abs()).max().item():.3e}; "
          f"ref {ref.flatten().tolist()}")
    assert got.shape == (B, 1, 1, 1) and (ref > 0).all()
    assert (err <= 2e-3 + 1e-2 * ref.abs()).all(), (got.flatten(), ref.flatten())


def test_exact_properties(weights):
    from view_neti_amd.engine.lpips import LPIPSEngine
    vgg, lin = weights
    H, W = 60, 84
    x, y = _images(6, H, W, 5), _images(6, H, W, 6)
    eng = LPIPSEngine(vgg, lin, H, W, max_images=12, device=DEV)
    assert (eng(x, x) == 0).all()
    d = eng(x, y)
    assert (d > 0).all() and torch.equal(d, eng(y, x)) and torch.equal(d, eng(x, y))
    # position in the batch (fixed batch size 4): pair 0 moved to the last slot
    a = eng(x[:4], y[:4])
    perm = torch.tensor([3, 1, 2, 0])
    b = eng(x[:4][perm], y[:4][perm])
    assert torch.equal(a, b[perm])
    # more pairs than max_images / 2: sub-batches of 2 pairs against one batch of 6
    small = LPIPSEngine(vgg, lin, H, W, max_images=4, device=DEV)
    assert torch.equal(small(x, y), d)
    # the shared-ground-truth form: features of the ground truth once, paired with each set of predictions
    preds = torch.stack([x, y])  # [S=2, V=6]
    gt = _images(6, H, W, 7)
    c = small.compare(preds, gt)
    assert torch.equal(c[0], eng(x, gt).flatten()) and torch.equal(c[1], eng(y, gt).flatten())


def test_refuses_bf16_and_non_finite(weights, monkeypatch):
    from view_neti_amd import lib
    from view_neti_amd.engine.lpips import LPIPSEngine
    vgg, lin = weights
    monkeypatch.setattr(lib, "_precision", "bf16")
    with pytest.raises(RuntimeError, match="fp16"):
        LPIPSEngine(vgg, lin, 32, 32, device=DEV)
    monkeypatch.undo()
    eng = LPIPSEngine(vgg, lin, 32, 32, max_images=2, device=DEV)
    x = _images(1, 32, 32, 8)
    with pytest.raises(FloatingPointError):
        eng(x * 1e6, x)  # 1e6 / 0.45 overflows f16 at the first convolution


def test_dtu_harness_with_lpips(tmp_path, weights):
    from PIL import Image
    from view_neti_amd.compat import dtu_metrics as dm
    from view_neti_amd.compat.dataset import TextualInversionDataset as DS
    from view_neti_amd.compat.lpips import LPIPS
    vgg, lin = weights
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    lpips_fn = LPIPS.from_files(tmp_path / "vgg16.pth", tmp_path / "vgg.pth")
    scene = tmp_path / "scan114"
    scene.mkdir()
    rng = np.random.default_rng(1)
    cam_idxs, cam_train, _ = dm.get_cam_idxs(3)
    for c in cam_idxs:
        low = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
        Image.fromarray(low).resize((160, 120), Image.BICUBIC).save(scene / DS.dtu_cam_and_lighting_to_fname(c, "3"))
    masks_root = tmp_path / "masks"
    (masks_root / "scan114" / "mask").mkdir(parents=True)
    m = np.zeros((1200, 1600, 3), np.uint8)
    m[300:900, 400:1200] = 255
    Image.fromarray(m).save(masks_root / "scan114" / "mask" / f"{cam_idxs[0]:03d}.png")
    gt = dm.dtu_get_gt_images(cam_idxs, scene, "3", 1)
    pred = {}
    for c in cam_idxs:
        a = np.asarray(gt[c]).astype(np.int32)
        noisy = np.clip(a + rng.integers(-40, 41, a.shape), 0, 255)
        pred[c] = np.stack([a if c in cam_train else noisy, noisy]).astype(np.uint8)  # seed 0 exact on train views
    res = dm.evaluate_dtu_predictions(pred, scene, 3, "3", 1, seeds=[0, 1], masks_root=str(masks_root),
                                      do_lpips=True, lpips_fn=lpips_fn, make_figures=False)
    assert 0 < res["lpips_train_mean"] < res["lpips_test_mean"]
    tr = torch.tensor([c in cam_train for c in cam_idxs])
    mk, g = res["masks"], res["imgs_gt"]
    # the argument order of dtu_metrics.lpips_fn_batch as get_result_metrics_and_grids calls it
    direct = [lpips_fn(g * mk * 2 - 1, p * mk * 2 - 1)[:, 0, 0, 0].cpu() for p in res["imgs_pred"]]
    assert (direct[0][tr] == 0).all() and (direct[1][tr] > 0).all()
    assert res["lpips_train_mean"] == torch.cat([d[tr] for d in direct]).mean().item()
    assert res["lpips_test_mean"] == torch.cat([d[~tr] for d in direct]).mean().item()
