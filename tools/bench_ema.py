"""Cost of the exponential moving average of the mappers on the train step, in one process: SD-1.5 shapes at
512^2, batch 4, synthetic weights — bench.py's engine, built once per arm with one set of autotuner picks:

    off               the step as it always was (the launch list of a run without ema_decay)
    ema               ema_decay: two launches more at the end of the optimizer step (prepare, apply) over one mapper
    off (control)     a second build of the `off` arm: the resolution of the comparison
    m3 off / m3 ema   the same pair over a bucket of `--objects` object mappers (learnable_mode 3's form, no view mapper:
                      the benchmark's batch has no view token) — the one case where the update moves real bytes, two reads
                      and one write of the whole bucket
    m3 off (control)  a second build of `m3 off`

All are captured graphs.  The arms are timed in alternation, a window of `--iters` steps each, `--repeats` times, each
window ending in a device synchronise.  Prints ms/step per arm and repeat, the update alone on the m3 bucket timed with
device events (launches back to back, outside the step), and one JSON line.  The achieved bytes/s of the m3 update is derived
from the arm difference, and the line says whether that difference is inside the control arm's spread.  There is no pass
bar: the comparison is the off arm of the same run.

    python tools/bench_ema.py [--model sd15] [--batch 4] [--resolution 512] [--iters 20] [--repeats 3] [--objects 88]
"""
import argparse
import contextlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_loss_options import window  # noqa: E402

MAPPER_OBJECT_ARG = 7  # position of `mapper_object` in TrainStepEngine's signature


@contextlib.contextmanager
def engine_arguments(objects=1, **kw):
    """bench.build_engine builds `view_neti_amd.engine.step.TrainStepEngine` around ONE mapper state: hand it the arm's
    extra arguments and, for the m3 arms, `objects` copies of that state as the bucket"""
    from view_neti_amd.engine import step
    orig = step.TrainStepEngine

    def build(*a, **k):
        a = list(a)
        if objects > 1:
            a[MAPPER_OBJECT_ARG] = [a[MAPPER_OBJECT_ARG]] * objects
        return orig(*a, **k, **kw)
    step.TrainStepEngine = build
    try:
        yield
    finally:
        step.TrainStepEngine = orig


def update_alone_us(eng, launches=200):
    """device time of one ema_update (prepare + apply) on the engine's own buffers, launches back to back; the engine's
    average is put back afterwards"""
    from view_neti_amd import ops
    keep = (eng.ema.clone(), eng.ema_count.clone())
    args = (eng.ema, eng.params, eng.opt_step, eng.ema_count, eng.ema_hyper, eng.ema_coef)
    eng.ema_count[1] = -1  # never equal to opt_step: every launch applies
    for _ in range(10):
        ops.ema_update(*args)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        eng.ema_count[1:].fill_(-1)
        ops.ema_update(*args)
    t1.record()
    t1.synchronize()
    with_fill = t0.elapsed_time(t1)
    t0.record()
    for _ in range(launches):
        eng.ema_count[1:].fill_(-1)
    t1.record()
    t1.synchronize()
    fill = t0.elapsed_time(t1)
    eng.ema.copy_(keep[0])
    eng.ema_count.copy_(keep[1])
    torch.cuda.synchronize()
    return (with_fill - fill) / launches * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--objects", type=int, default=88)
    ap.add_argument("--ema_decay", type=float, default=0.9999)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema needs a GPU")
    if not 1 < args.objects <= 88:
        raise SystemExit("--objects: 2..88 (the reference's largest run trains 88 scenes)")
    ema = dict(ema_decay=args.ema_decay)
    arms = {"off": {}, "ema": ema, "off (control)": {}, "m3 off": dict(objects=args.objects),
            "m3 ema": dict(objects=args.objects, **ema), "m3 off (control)": dict(objects=args.objects)}
    engines = {}
    for name, kw in arms.items():
        with engine_arguments(**kw):
            _, eng = bench.build_engine(args, 0, 1)
        eng.capture()
        for _ in range(3):
            eng.step()
        engines[name] = eng
    m3 = engines["m3 ema"]
    assert m3.n_objects == args.objects and engines["ema"].n_objects == 1 and engines["off"].ema is None
    print(f"m3 arms: {m3.n_objects} object mappers, a bucket of {m3.params.numel()} floats "
          f"({m3.params.numel() * 4 / 2 ** 20:.1f} MiB); one mapper: {engines['ema'].params.numel()} floats")
    ms = {name: [] for name in arms}
    for r in range(args.repeats):
        for name, eng in engines.items():
            ms[name].append(window(eng, args.iters))
        print(f"repeat {r}: " + "   ".join(f"{name} {ms[name][-1]:.3f} ms/step" for name in arms))
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    spread = lambda a, b: max(ms[a] + ms[b]) - min(ms[a] + ms[b])  # of two engines that enqueue the same launches
    moved = 3 * m3.params.numel() * 4  # two reads and one write of the bucket
    diff_us = (med["m3 ema"] - med["m3 off"]) * 1e3
    spread_us = spread("m3 off", "m3 off (control)") * 1e3
    alone_us = {"one mapper": update_alone_us(engines["ema"]), "m3": update_alone_us(m3)}
    out = {"model": args.model, "batch": args.batch, "resolution": args.resolution, "iters": args.iters,
           "objects": args.objects, "bucket_floats": m3.params.numel(),
           "ms_per_step": {k: round(v, 3) for k, v in med.items()},
           "ms_per_step_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "ema_over_off_us": round((med["ema"] - med["off"]) * 1e3, 1),
           "control_over_off_us": round((med["off (control)"] - med["off"]) * 1e3, 1),
           "off_spread_us": round(spread("off", "off (control)") * 1e3, 1),
           "m3_ema_over_off_us": round(diff_us, 1),
           "m3_control_over_off_us": round((med["m3 off (control)"] - med["m3 off"]) * 1e3, 1),
           "m3_off_spread_us": round(spread_us, 1),
           "m3_difference_inside_control_spread": bool(abs(diff_us) <= spread_us),
           "m3_update_bytes": moved,
           "m3_update_GBps_from_arm_difference": round(moved / (diff_us * 1e-6) / 1e9, 1) if diff_us > 0 else None,
           "update_alone_us": {k: round(v, 2) for k, v in alone_us.items()},
           "m3_update_alone_GBps": round(moved / (alone_us["m3"] * 1e-6) / 1e9, 1),
           "ema_updates": {k: int(e.ema_count[0]) for k, e in engines.items() if e.ema is not None},
           "losses": {k: round(e.loss(), 6) for k, e in engines.items()},
           "params_finite": all(bool(torch.isfinite(e.params).all()) for e in engines.values())}
    if out["m3_difference_inside_control_spread"]:
        print(f"the m3 difference ({diff_us:.1f} us) is INSIDE the spread of the two m3 off engines ({spread_us:.1f} us): "
              "the bytes/s derived from it is not resolved")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
