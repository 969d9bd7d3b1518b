"""Cost of the object-masked loss on the train step, in one process: SD-1.5 shapes at 512^2, batch 4,
synthetic weights — bench.py's engine, built once per arm with one set of autotuner picks:

    off            the step as it always was (the launch list of a run without data.mask_dir)
    mask           loss_mask: the weighted loss entry in place of the plain one, no launch more; the weight table holds the
                   rows of four random masks, written once before the windows (the step only reads it)
    off (control)  a second build of the `off` arm: the difference between two engines that enqueue the same launches is the
                   resolution of the comparison

All are captured graphs.  The arms are timed in alternation, a window of `--iters` steps each, `--repeats` times, each
window ending in a device synchronise.  Then the preparation entry alone — vneti_loss_weights_from_mask, both launches,
what a run pays per sample and step OUTSIDE the captured step — `--prep_calls` calls back to back between two device
events, from a 512^2 mask at pixel stride 1 (the host path's upload) and 3 (the device input pipeline's buffer).  Prints
ms/step per arm and repeat, and one JSON line.  There is no pass bar: the comparison is the off arm of the same run.

    python tools/bench_loss_mask.py [--model sd15] [--batch 4] [--resolution 512] [--iters 20] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_telemetry import engine_arguments  # noqa: E402


def window(eng, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def random_masks(batch, res, seed=0):
    """uint8 [batch][res][res]: a disc of random centre and radius per sample (the object), 255 inside"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
    out = []
    for _ in range(batch):
        cx, cy = (torch.rand(2, generator=g) * 0.4 + 0.3) * res
        r = (torch.rand(1, generator=g) * 0.2 + 0.15) * res
        out.append((((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r).to(torch.uint8) * 255)
    return torch.stack(out)


def time_preparation(eng, res, calls):
    """us per vneti_loss_weights_from_mask call (two launches), device events around `calls` calls back to back"""
    out = {}
    mask = random_masks(1, res, seed=1)[0]
    for stride in (1, 3):
        img = (mask if stride == 1 else mask[:, :, None].expand(res, res, 3)).contiguous().cuda()
        for _ in range(10):
            eng.set_loss_mask(0, img, res, res, stride)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            eng.set_loss_mask(0, img, res, res, stride)
        b.record()
        torch.cuda.synchronize()
        out[f"stride{stride}"] = round(a.elapsed_time(b) / calls * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--background", type=float, default=0.0)
    ap.add_argument("--prep_calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_mask needs a GPU")
    arms = {"off": {}, "mask": dict(loss_mask=True, loss_mask_background=args.background), "off (control)": {}}
    engines = {}
    for name, kw in arms.items():
        with engine_arguments(**kw):
            _, eng = bench.build_engine(args, 0, 1)
        if eng.loss_weights is not None:
            eng.set_loss_masks(random_masks(args.batch, args.resolution))
        eng.capture()
        for _ in range(3):
            eng.step()
        engines[name] = eng
    ms = {name: [] for name in arms}
    for r in range(args.repeats):
        for name, eng in engines.items():
            ms[name].append(window(eng, args.iters))
        print(f"repeat {r}: " + "   ".join(f"{name} {ms[name][-1]:.3f} ms/step" for name in arms))
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    prep = time_preparation(engines["mask"], args.resolution, args.prep_calls)
    print(f"preparation alone, {args.prep_calls} calls back to back: " + "   ".join(f"{k} {v} us" for k, v in prep.items()))
    q = engines["mask"].loss_weights
    out = {"model": args.model, "batch": args.batch, "resolution": args.resolution, "iters": args.iters,
           "ms_per_step": {k: round(v, 3) for k, v in med.items()},
           "ms_per_step_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "mask_over_off_us": round((med["mask"] - med["off"]) * 1e3, 1),
           "control_over_off_us": round((med["off (control)"] - med["off"]) * 1e3, 1),
           "preparation_us_per_sample": prep,
           "weights_mean": round(float(q.mean()), 6), "weights_zero_fraction": round(float((q == 0).float().mean()), 4),
           "losses": {k: round(e.loss(), 6) for k, e in engines.items()},
           "params_finite": all(bool(torch.isfinite(e.params).all()) for e in engines.values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
