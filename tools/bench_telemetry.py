"""Cost of the per-step training record and of gradient-norm clipping on the train step, in one process:
SD-1.5 shapes at 512^2, batch 4, synthetic weights — bench.py's engine, built once per arm with one set of autotuner picks:

    off            the step as it always was (the launch list of a run that uses neither)
    record         telemetry_rows > 0
    record + clip  telemetry_rows > 0 and max_grad_norm

All are captured graphs.  The arms are timed in alternation, a window of `--iters` steps each, `--repeats` times, each
window ending in a device synchronise.  The record arms then read the ring (read_telemetry(), as Coach does at its log
point, every 50 steps there); that read is timed on its own, after the window.  A fourth engine, `off (control)`, is a
second build of the `off` arm: the difference between two engines that enqueue the same launches is the resolution of the
comparison.  Prints ms/step per arm and repeat, ms per read, and one JSON line.

    python tools/bench_telemetry.py [--model sd15] [--batch 4] [--resolution 512] [--iters 20] [--repeats 3]
"""
import argparse
import contextlib
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


@contextlib.contextmanager
def engine_arguments(**kw):
    """bench.build_engine builds `view_neti_amd.engine.step.TrainStepEngine`: hand it the arm's extra arguments"""
    from view_neti_amd.engine import step
    orig = step.TrainStepEngine
    step.TrainStepEngine = functools.partial(orig, **kw)
    try:
        yield
    finally:
        step.TrainStepEngine = orig


def window(eng, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    read_ms = None
    if eng.telemetry_rows:
        t0 = time.perf_counter()
        rows, lost = eng.read_telemetry()
        read_ms = (time.perf_counter() - t0) * 1e3
        assert len(rows) == iters and lost == 0 and all(r["closed"] for r in rows)
    return ms, read_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_telemetry needs a GPU")
    arms = {"off": {}, "record": dict(telemetry_rows=2 * args.iters),
            "record+clip": dict(telemetry_rows=2 * args.iters, max_grad_norm=args.max_grad_norm), "off (control)": {}}
    engines = {}
    for name, kw in arms.items():
        with engine_arguments(**kw):
            _, eng = bench.build_engine(args, 0, 1)
        eng.capture()
        for _ in range(3):
            eng.step()
        if eng.telemetry_rows:
            eng.read_telemetry()
        engines[name] = eng
    ms, reads = {name: [] for name in arms}, []
    for r in range(args.repeats):
        for name, eng in engines.items():
            t, read_ms = window(eng, args.iters)
            ms[name].append(t)
            if read_ms is not None:
                reads.append(read_ms)
        print(f"repeat {r}: " + "   ".join(f"{name} {ms[name][-1]:.3f} ms/step" for name in arms))
    print(f"read_telemetry() of {args.iters} rows: " + " ".join(f"{x:.3f}" for x in reads) + " ms")
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    out = {"model": args.model, "batch": args.batch, "resolution": args.resolution, "iters": args.iters,
           "ms_per_step": {k: round(v, 3) for k, v in med.items()},
           "ms_per_step_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "record_over_off_us": round((med["record"] - med["off"]) * 1e3, 1),
           "record_clip_over_off_us": round((med["record+clip"] - med["off"]) * 1e3, 1),
           "control_over_off_us": round((med["off (control)"] - med["off"]) * 1e3, 1),
           "read_ms": round(sorted(reads)[len(reads) // 2], 3),
           "params_finite": all(bool(torch.isfinite(e.params).all()) for e in engines.values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
