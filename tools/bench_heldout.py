"""Time of one held-out evaluation batch (TrainStepEngine.eval_losses) beside the train step of the SAME
engine, in one process: SD-1.5 shapes at 512^2, batch 4, synthetic weights.  Both are captured graphs; eval_losses() and
step() are timed in alternation (a window of `--iters` calls of one, then of the other), `--repeats` times, each window
ending in a device synchronise.  eval_losses() includes what a caller pays per batch: the replay, the device -> host copy
of B floats and the synchronise.

Prints the windows and one JSON line: ms per evaluation batch, its ratio to the train step, and the time of a full
34-view x K = 4 evaluation (136 items = 34 batches of 4) without the host-side input preparation.  The evaluation's launch
list is a strict subset of the step's: a ratio at or above 1 is a bug, and the tool exits non-zero on it.

    python tools/bench_heldout.py [--model sd15] [--batch 4] [--resolution 512] [--iters 20] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--views", type=int, default=34)
    ap.add_argument("--timesteps", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heldout needs a GPU")
    cfg, eng = bench.build_engine(args, 0, 1)
    eng.capture()
    for _ in range(3):  # warm both graphs (the first eval_losses() captures graph_eval)
        eng.step()
        eng.eval_losses()
    ev, st = [], []
    for r in range(args.repeats):
        ev.append(window(eng.eval_losses, args.iters))
        st.append(window(eng.step, args.iters))
        print(f"repeat {r}: eval batch {ev[-1]:.3f} ms   train step {st[-1]:.3f} ms   ratio {ev[-1] / st[-1]:.3f}")
    ev_ms, st_ms = sorted(ev)[len(ev) // 2], sorted(st)[len(st) // 2]
    n_batches = -(-args.views * args.timesteps // args.batch)
    out = {"model": args.model, "batch": args.batch, "resolution": args.resolution, "iters": args.iters,
           "eval_batch_ms": round(ev_ms, 3), "train_step_ms": round(st_ms, 3), "eval_over_step": round(ev_ms / st_ms, 4),
           "eval_batch_ms_all": [round(x, 3) for x in ev], "train_step_ms_all": [round(x, 3) for x in st],
           "full_eval_batches": n_batches, "full_eval_s": round(n_batches * ev_ms / 1e3, 3),
           "loss_finite": bool(torch.isfinite(eng.eval_losses()).all())}
    print(json.dumps(out))
    if not ev_ms < st_ms:
        raise SystemExit("the evaluation batch is not faster than the train step of the same engine: a bug to find")


if __name__ == "__main__":
    main()
