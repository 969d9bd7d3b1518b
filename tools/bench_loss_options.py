"""Cost of Min-SNR loss weighting and of offset noise on the train step, in one process: SD-1.5 shapes at
512^2, batch 4, synthetic weights — bench.py's engine, built once per arm with one set of autotuner picks:

    off            the step as it always was (the launch list of a run that uses neither)
    snr            snr_gamma: the weighted loss entry in place of the plain one, no launch more
    snr + offset   snr_gamma and noise_offset: one rng_fill_normal of B x 4 values more, the offset entry in place of the plain

All are captured graphs.  The arms are timed in alternation, a window of `--iters` steps each, `--repeats` times, each
window ending in a device synchronise.  A fourth engine, `off (control)`, is a second build of the `off` arm: the difference
between two engines that enqueue the same launches is the resolution of the comparison.  Prints ms/step per arm and repeat,
and one JSON line.  There is no pass bar: the comparison is the off arm of the same run.

    python tools/bench_loss_options.py [--model sd15] [--batch 4] [--resolution 512] [--iters 20] [--repeats 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--snr_gamma", type=float, default=5.0)
    ap.add_argument("--noise_offset", type=float, default=0.1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_options needs a GPU")
    arms = {"off": {}, "snr": dict(snr_gamma=args.snr_gamma),
            "snr+offset": dict(snr_gamma=args.snr_gamma, noise_offset=args.noise_offset), "off (control)": {}}
    engines = {}
    for name, kw in arms.items():
        with engine_arguments(**kw):
            _, eng = bench.build_engine(args, 0, 1)
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
    out = {"model": args.model, "batch": args.batch, "resolution": args.resolution, "iters": args.iters,
           "ms_per_step": {k: round(v, 3) for k, v in med.items()},
           "ms_per_step_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "snr_over_off_us": round((med["snr"] - med["off"]) * 1e3, 1),
           "snr_offset_over_off_us": round((med["snr+offset"] - med["off"]) * 1e3, 1),
           "control_over_off_us": round((med["off (control)"] - med["off"]) * 1e3, 1),
           "losses": {k: round(e.loss(), 6) for k, e in engines.items()},
           "params_finite": all(bool(torch.isfinite(e.params).all()) for e in engines.values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
