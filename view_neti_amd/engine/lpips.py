"""LPIPS(net="vgg", version="0.1") on the GPU: the perceptual distance of the DTU novel-view metrics.

Restates lpips 0.1.4 in eval mode (lpips/lpips.py `LPIPS.forward`, pretrained_networks.py `vgg16`) as the reference
constructs it (training/inference_dtu.py `LPIPS(net="vgg")`, scripts/summarize_dtu.py):

  x' = (x - shift) / scale                               ScalingLayer, x in [-1, 1]
  VGG16 features: 13 3x3 pad-1 convolutions + bias + ReLU, 2x2 max-pools, taps relu1_2 .. relu5_3
  per tap k and pixel: n = f / (|f|_2 + 1e-10) over channels, d = sum_c w_k[c] (n0_c - n1_c)^2, spatial mean
  LPIPS = sum over the five taps

The convolutions are vneti_gemm_f16 launches (conv1_1 as a plain GEMM over the scaled 3-channel im2col of
vneti_lpips_prep, the others as implicit convolutions, conv_mode 1) with a tile pinned per stage and no split-K, so an
image's features do not depend on the batch it is computed in.  ReLU, ReLU + max-pool and the distance are the kernels of
csrc/lpips.hip.  Features are computed once per image: `distance(pairs)` compares any (i, j) of the loaded batch, so a
ground truth shared by several predictions is run once.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .. import lib, ops, packing

# features.<index> of torchvision's vgg16 for the 13 convolutions, grouped by stage (a 2x2 max-pool between stages)
VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256),
                (256, 512), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512))
STAGES = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))  # conv positions; the last of each stage is tapped
TAP_CHANNELS = (64, 128, 256, 512, 512)
# GEMM tile per stage (vneti_gemm_desc.tile_hint): 128x64 for the 64-channel stage, the 256x128 8-phase tile where there
# are many pixels, 128x128 on the small deep stages.  Pinned, not chosen from M, so results do not depend on the batch.
STAGE_TILE = (2, 17, 17, 1, 1)
BUFFER_LIMIT = 0x7fffffff  # every store through a buffer resource stays below 2 GiB


class LPIPSEngine:
    """LPIPS-VGG for images of one size H x W, at most `max_images` feature images per pass (larger requests are cut)."""

    def __init__(self, vgg_state: Dict[str, torch.Tensor], lin_state: Dict[str, torch.Tensor], H: int, W: int,
                 max_images: int = 32, device="cuda"):
        if lib.precision() != "fp16":
            raise RuntimeError("LPIPS runs on the fp16 library only: its quality with bf16 operands is unmeasured "
                               f"(this process computes in {lib.precision()})")
        if H < 16 or W < 16:
            raise ValueError(f"LPIPS-VGG needs images of at least 16 x 16 (four 2x2 pools), got {H} x {W}")
        self.H, self.W, self.max_images = int(H), int(W), int(max_images)
        self.device = torch.device(device)
        dev, f16 = self.device, lib.act_dtype()
        if self.max_images < 2:
            raise ValueError("max_images must be >= 2 (one pair)")
        # stage geometry: (H, W) of each stage's convolutions (floor pooling)
        self.geom = []
        h, w = self.H, self.W
        for s in range(5):
            self.geom.append((h, w))
            h, w = h // 2, w // 2
        per_image = self.H * self.W * 64 * 2  # the largest activation: 64 channels at full size
        if self.max_images * per_image >= BUFFER_LIMIT:
            raise ValueError(f"max_images={self.max_images}: {self.max_images * per_image} bytes of activations per "
                             f"buffer, over the 2 GiB limit of the buffer stores; at {H} x {W} at most "
                             f"{(BUFFER_LIMIT - 1) // per_image}")
        # weights: B [Co][K] 16-bit in the GEMM's K order (tap, channel), f32 biases
        self.wts, self.bias = [], []
        for n, (i, (ci, co)) in enumerate(zip(VGG_CONV_INDEX, VGG_CHANNELS)):
            wt = vgg_state[f"features.{i}.weight"].detach().float().cpu()
            pk = packing.conv3x3_fwd(wt, cm=False)
            if n == 0:
                pk = packing.pad_rows(pk, 64)  # K = 27 -> 64, matching the zero columns of vneti_lpips_prep
            self.wts.append(pk.to(dev, f16).contiguous())
            self.bias.append(vgg_state[f"features.{i}.bias"].detach().float().to(dev).contiguous())
        self.lin = [lin_state[f"lin{k}.model.1.weight"].detach().float().reshape(-1).to(dev).contiguous()
                    for k in range(5)]
        n = self.max_images
        big = n * self.H * self.W * 64
        self.scratch = [torch.empty(big, dtype=f16, device=dev), torch.empty(big, dtype=f16, device=dev)]
        self.taps = [torch.empty(n * h * w * c, dtype=f16, device=dev) for (h, w), c in zip(self.geom, TAP_CHANNELS)]
        self.n_loaded = 0

    # ------------------------------------------------------------------------------------------------ features
    def _conv(self, idx, src, dst, n, h, w, tile):
        ci, co = VGG_CHANNELS[idx]
        M = n * h * w
        out = dst[:M * co].view(M, co)
        if idx == 0:
            ops.gemm(src[:M * 64].view(M, 64), self.wts[0], out, bias=self.bias[0], tile_hint=tile, split_k=1)
        else:
            ops.gemm(src, self.wts[idx], out, bias=self.bias[idx], tile_hint=tile, split_k=1, M=M, N=co, K=9 * ci,
                     conv=dict(mode=1, Hi=h, Wi=w, Ci=ci, Ho=h, Wo=w, stride=1, pad_t=1, pad_l=1, ups=0, ldx=ci))

    @torch.no_grad()
    def features(self, imgs: torch.Tensor) -> None:
        """run VGG16 on n <= max_images images (n, 3, H, W) in [-1, 1]; keeps the five tapped pre-activations"""
        if imgs.dim() != 4 or imgs.shape[1] != 3 or tuple(imgs.shape[2:]) != (self.H, self.W):
            raise ValueError(f"expected (n, 3, {self.H}, {self.W}) images, got {tuple(imgs.shape)}")
        n = imgs.shape[0]
        if not 1 <= n <= self.max_images:
            raise ValueError(f"{n} images, the engine holds 1..{self.max_images}")
        x = imgs.to(self.device, torch.float32)
        a, b = self.scratch
        ops.lpips_prep(x, a, n, self.H, self.W)
        cur, other = a, b
        for s, convs in enumerate(STAGES):
            h, w = self.geom[s]
            for idx in convs:
                last = idx == convs[-1]
                dst = self.taps[s] if last else other
                self._conv(idx, cur, dst, n, h, w, STAGE_TILE[s])
                if last:
                    if s < 4:
                        ops.relu_maxpool2x2(self.taps[s], cur, n, h, w, VGG_CHANNELS[idx][1])
                else:
                    ops.relu_(dst[:n * h * w * VGG_CHANNELS[idx][1]])
                    cur, other = dst, cur
        self.n_loaded = n

    @torch.no_grad()
    def distance(self, pairs) -> torch.Tensor:
        """LPIPS of the loaded feature images pairs[p] = (i, j): f32 [P] on the device"""
        pairs = torch.as_tensor(pairs, dtype=torch.int32).reshape(-1, 2)
        if pairs.numel() == 0:
            return torch.zeros(0, dtype=torch.float32, device=self.device)
        if int(pairs.min()) < 0 or int(pairs.max()) >= self.n_loaded:
            raise ValueError(f"pair indices must lie in [0, {self.n_loaded}), the loaded feature batch")
        pairs = pairs.to(self.device).contiguous()
        P = pairs.shape[0]
        out = torch.empty(P, dtype=torch.float32, device=self.device)
        ws_n = max(ops.lpips_ws_floats(P, c, h * w) for (h, w), c in zip(self.geom, TAP_CHANNELS))
        ws = torch.empty(ws_n, dtype=torch.float32, device=self.device)
        for k, ((h, w), c) in enumerate(zip(self.geom, TAP_CHANNELS)):
            ops.lpips_distance(self.taps[k], self.n_loaded, pairs, self.lin[k], c, h * w, ws, out, accumulate=k > 0)
        return out

    @staticmethod
    def _finite(out: torch.Tensor) -> torch.Tensor:
        if not bool(torch.isfinite(out).all()):
            raise FloatingPointError("LPIPS produced a non-finite value (an f16 overflow in the VGG features?)")
        return out

    # ------------------------------------------------------------------------------------------------ requests
    @torch.no_grad()
    def pairs(self, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
        """LPIPS(in0[b], in1[b]) for (B, 3, H, W) batches in [-1, 1]: f32 [B] on the device"""
        if in0.shape != in1.shape:
            raise ValueError(f"shape mismatch {tuple(in0.shape)} vs {tuple(in1.shape)}")
        B = in0.shape[0]
        step = self.max_images // 2
        outs: List[torch.Tensor] = []
        for s in range(0, B, step):
            m = min(step, B - s)
            self.features(torch.cat((in0[s:s + m].to(self.device), in1[s:s + m].to(self.device))))
            outs.append(self.distance([(k, m + k) for k in range(m)]))
        return self._finite(torch.cat(outs))

    @torch.no_grad()
    def compare(self, preds: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """LPIPS(preds[s, v], gt[v]) for S prediction sets of the same V views, in [-1, 1]: f32 [S, V] on the device; the
        ground-truth features are computed once per view, not once per set"""
        S, V = preds.shape[:2]
        if tuple(preds.shape[1:]) != tuple(gt.shape):
            raise ValueError(f"predictions {tuple(preds.shape)} vs ground truth {tuple(gt.shape)}")
        step = self.max_images // (S + 1)
        if step < 1:
            raise ValueError(f"{S} prediction sets need max_images >= {S + 1}")
        out = torch.empty(S, V, dtype=torch.float32, device=self.device)
        for v0 in range(0, V, step):
            m = min(step, V - v0)
            imgs = [gt[v0:v0 + m].to(self.device)] + [preds[s, v0:v0 + m].to(self.device) for s in range(S)]
            self.features(torch.cat(imgs))
            pairs = [((s + 1) * m + k, k) for s in range(S) for k in range(m)]
            out[:, v0:v0 + m] = self.distance(pairs).view(S, m)
        return self._finite(out)

    def __call__(self, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
        """the lpips.LPIPS call contract: (B, 1, 1, 1) f32"""
        return self.pairs(in0, in1).view(-1, 1, 1, 1)

    @staticmethod
    def flops_per_image(H: int, W: int) -> float:
        """multiply-adds x 2 of the 13 convolutions at H x W"""
        total, h, w = 0.0, H, W
        for s, convs in enumerate(STAGES):
            for idx in convs:
                ci, co = VGG_CHANNELS[idx]
                total += 2.0 * h * w * co * 9 * ci
            h, w = h // 2, w // 2
        return total
