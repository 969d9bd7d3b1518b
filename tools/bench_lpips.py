"""Dev tool: LPIPS-VGG throughput at the DTU evaluation size (300x400) for one scene's worth of work — 34 views x 2 seeds
against a shared ground truth (102 feature images, 68 pairs) — on the GPU (engine/lpips.py, `compare`), and the fp32 host
restatement (tests/helpers/lpips_ref.py) with threads capped to the cgroup quota as bench.py does.  Synthetic seeded
weights.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import torch  # noqa: E402

import lpips_ref  # noqa: E402
from bench import usable_cores  # noqa: E402
from view_neti_amd.engine.lpips import LPIPSEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=34)
ap.add_argument("--seeds", type=int, default=2)
ap.add_argument("--H", type=int, default=300)
ap.add_argument("--W", type=int, default=400)
ap.add_argument("--max_images", type=int, default=102)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--host_images", type=int, default=2, help="images the host restatement runs (its time is scaled)")
a = ap.parse_args()

vgg, lin = lpips_ref.synthetic_weights(0)
g = torch.Generator().manual_seed(0)
gt = torch.rand(a.views, 3, a.H, a.W, generator=g) * 2 - 1
preds = (gt.unsqueeze(0) + 0.2 * torch.randn(a.seeds, a.views, 3, a.H, a.W, generator=g)).clamp(-1, 1)
n_img = a.views * (a.seeds + 1)
n_pairs = a.views * a.seeds
flop = LPIPSEngine.flops_per_image(a.H, a.W) * n_img

eng = LPIPSEngine(vgg, lin, a.H, a.W, max_images=a.max_images, device="cuda")
gt_d, preds_d = gt.cuda(), preds.cuda()
out = eng.compare(preds_d, gt_d)  # warm-up: code objects, allocations
torch.cuda.synchronize()
times = []
for _ in range(a.repeats):
    t0 = time.perf_counter()
    eng.compare(preds_d, gt_d)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
t_gpu = sorted(times)[len(times) // 2]

cores = usable_cores()
torch.set_num_threads(cores)
k = a.host_images
t0 = time.perf_counter()
lpips_ref.lpips(preds[0, :k // 2 or 1], gt[:k // 2 or 1], vgg, lin)
t_host_k = time.perf_counter() - t0
t_host = t_host_k / (2 * (k // 2 or 1)) * n_img  # per image (features dominate) x the scene's images

print(json.dumps(dict(
    metric="lpips_vgg_scene", size=f"{a.H}x{a.W}", views=a.views, seeds=a.seeds, feature_images=n_img, pairs=n_pairs,
    gpu_s=round(t_gpu, 5), gpu_pairs_per_s=round(n_pairs / t_gpu, 1), gpu_tflops=round(flop / t_gpu / 1e12, 1),
    gflop_per_image=round(LPIPSEngine.flops_per_image(a.H, a.W) / 1e9, 2), host_threads=cores,
    host_s_scene=round(t_host, 2), host_images_timed=2 * (k // 2 or 1), speedup=round(t_host / t_gpu, 1),
    gpu_repeats=[round(t, 5) for t in times], finite=bool(torch.isfinite(out).all()))))
