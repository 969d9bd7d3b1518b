"""`lpips.LPIPS(net="vgg")` from user-supplied weight files, on the GPU (engine/lpips.py).

    lpips_fn = LPIPS.from_files("vgg16-397923af.pth", "lpips/weights/v0.1/vgg.pth")
    d = lpips_fn(pred, gt)[:, 0, 0, 0]          # pred, gt: (B, 3, H, W) in [-1, 1]
    dtu_metrics.lpips_fn_batch(imgs_gt, imgs_pred, lpips_fn=lpips_fn)

Two files, both explicit paths; nothing is searched for or downloaded:
  * torchvision's VGG16 state dict (`vgg16-397923af.pth`): features.{0,2,5,...,28}.{weight,bias}
  * the lpips package's linear heads (`weights/v0.1/vgg.pth`): lin{0..4}.model.1.weight, (1, C, 1, 1)
The loaders check every key and shape and run without a GPU.  Parity is pinned to the published algorithm of lpips 0.1.4
(tests/helpers/lpips_ref.py restates it step by step), not to the package itself, which is not available here.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Union

import torch

from ..engine.lpips import TAP_CHANNELS, VGG_CHANNELS, VGG_CONV_INDEX

PathLike = Union[str, Path]


def _load_state(path: PathLike) -> Dict[str, torch.Tensor]:
    path = Path(path)
    if not path.is_file():
        raise FileNotFoundError(f"LPIPS weight file {path} does not exist")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _check(sd: Dict[str, torch.Tensor], expected: Dict[str, tuple], what: str) -> Dict[str, torch.Tensor]:
    out = {}
    for key, shape in expected.items():
        if key not in sd:
            raise KeyError(f"{what}: missing key {key!r}")
        t = sd[key]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: key {key!r} has shape {got}, expected {shape}")
        out[key] = t.detach().float()
    return out


def vgg_expected() -> Dict[str, tuple]:
    keys = {}
    for i, (ci, co) in zip(VGG_CONV_INDEX, VGG_CHANNELS):
        keys[f"features.{i}.weight"] = (co, ci, 3, 3)
        keys[f"features.{i}.bias"] = (co,)
    return keys


def lin_expected() -> Dict[str, tuple]:
    return {f"lin{k}.model.1.weight": (1, c, 1, 1) for k, c in enumerate(TAP_CHANNELS)}


def load_vgg16_features(path_or_state) -> Dict[str, torch.Tensor]:
    """torchvision vgg16 state dict (a path or the dict) -> the 26 convolution tensors of `features`, f32 on the host"""
    sd = path_or_state if isinstance(path_or_state, dict) else _load_state(path_or_state)
    return _check(sd, vgg_expected(), "VGG16 weights")


def load_lpips_lin(path_or_state) -> Dict[str, torch.Tensor]:
    """lpips v0.1 vgg.pth (a path or the dict) -> the five linear heads, f32 on the host"""
    sd = path_or_state if isinstance(path_or_state, dict) else _load_state(path_or_state)
    return _check(sd, lin_expected(), "LPIPS linear heads")


class LPIPS:
    """The `lpips.LPIPS(net="vgg", version="0.1")` call contract on the HIP engine: `lpips_fn(in0, in1)` -> (B, 1, 1, 1)
    f32 (on the inputs' device).  One engine per image size, built on first use."""

    def __init__(self, vgg_state: Dict[str, torch.Tensor], lin_state: Dict[str, torch.Tensor], device="cuda",
                 max_images: int = 32):
        self.vgg = load_vgg16_features(vgg_state)
        self.lin = load_lpips_lin(lin_state)
        self.device = device
        self.max_images = max_images
        self._engines = {}

    @classmethod
    def from_files(cls, vgg_path: PathLike, lin_path: PathLike, device="cuda", max_images: int = 32) -> "LPIPS":
        return cls(load_vgg16_features(vgg_path), load_lpips_lin(lin_path), device=device, max_images=max_images)

    def engine(self, H: int, W: int):
        from ..engine.lpips import LPIPSEngine
        key = (int(H), int(W))
        if key not in self._engines:
            n = min(self.max_images, max(2, (0x7fffffff - 1) // (H * W * 64 * 2)))
            self._engines[key] = LPIPSEngine(self.vgg, self.lin, H, W, max_images=n, device=self.device)
        return self._engines[key]

    def __call__(self, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
        out = self.engine(*in0.shape[-2:])(in0, in1)
        return out.to(in0.device)

    def compare(self, preds: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """LPIPS(preds[s, v], gt[v]) -> [S, V] on the host; the ground truth's features are computed once per view"""
        return self.engine(*gt.shape[-2:]).compare(preds, gt).cpu()
