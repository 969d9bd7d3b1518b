"""Host side of the per-step training record (extension): a dump of the device ring -> rows.  Pure
functions on CPU tensors, no GPU.

The ring (include/vneti.h, VNETI_TELEMETRY_*) has `rows` rows of HEADER + 2 B floats, one per micro-step; micro-step c
(counting from 0) lives in row c % rows and carries c mod 2^24 as its sequence number.  vneti_train_record writes the
micro-step's part (sequence number, micro index, timesteps, per-sample losses), vneti_grad_norm_finish the optimizer's part
into the row of the micro-step that closed an accumulation group."""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

(SEQ, MICRO, CLOSED, NORM_OBJECT, NORM_VIEW, NORM_TOTAL, FINITE, CLIP_COEF, LOSS_SCALE, LR, HEADER) = range(11)
SEQ_MASK = 0xFFFFFF


def row_floats(batch: int) -> int:
    return HEADER + 2 * batch


def default_rows(steps: int, grad_accum: int) -> int:
    """a ring for reads every `steps` optimizer steps: twice the micro-steps between two reads"""
    return 2 * steps * grad_accum


def decode_ring(ring: torch.Tensor, count: int, last_read: int, batch: int) -> Tuple[List[Dict], int]:
    """ring: CPU f32 [rows, HEADER + 2 * batch] as copied from the device when the counter read `count`; last_read: the
    counter at the previous read.  -> (the micro-steps last_read .. count - 1 that are still in the ring, oldest first, as
    dicts; the number of them that are gone).  More than `rows` micro-steps since the last read: the oldest were
    overwritten.  A row whose sequence number is not the expected one belongs to another lap of the ring and counts as
    lost, never as data."""
    rows = ring.shape[0]
    assert ring.shape[1] == row_floats(batch) and 0 <= last_read <= count
    first = max(last_read, count - rows)
    out, lost = [], first - last_read
    for c in range(first, count):
        r = ring[c % rows].tolist()
        if int(r[SEQ]) != (c & SEQ_MASK):
            lost += 1
            continue
        d = {"micro_step": c, "micro": int(r[MICRO]), "timesteps": [int(x) for x in r[HEADER:HEADER + batch]],
             "losses": r[HEADER + batch:HEADER + 2 * batch], "closed": r[CLOSED] != 0.0}
        if d["closed"]:
            d.update(finite=r[FINITE] != 0.0, skipped=r[FINITE] == 0.0, clip_coef=r[CLIP_COEF], loss_scale=r[LOSS_SCALE],
                     lr=r[LR], grad_norm={"total": r[NORM_TOTAL]})
            # an absent side (no such mapper in the gradient bucket) is marked -1 by the device
            if not r[NORM_OBJECT] == -1.0:
                d["grad_norm"]["object"] = r[NORM_OBJECT]
            if not r[NORM_VIEW] == -1.0:
                d["grad_norm"]["view"] = r[NORM_VIEW]
        out.append(d)
    return out, lost


def finite_or_none(x: float):
    """JSON has no inf / nan: the norm of a skipped step is written as null"""
    return x if math.isfinite(x) else None
