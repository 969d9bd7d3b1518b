"""The optimizer restatement the AdamW kernel tests share (tests/test_optim_rng_gpu.py, tests/test_grad_norm_gpu.py): the
f32-rounded hyper-parameters the kernels read, torch.optim.AdamW driven with them, GradScaler's update rule restated in
`Scaler`, the spread gradients, and the sizes and activity pattern of the flat and the segmented bucket."""
import numpy as np
import torch

from helpers.checks import DEV, gen as _gen


def f32(x):
    return float(np.float32(x))


def i32(*vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


B1, B2, ADAM_EPS = f32(0.9), f32(0.999), f32(1e-8)


def hyper_dev(lr, wd, gdiv):
    return torch.tensor([lr, B1, B2, ADAM_EPS, wd, gdiv], dtype=torch.float32, device=DEV)


def torch_adamw(params, lr, wd):
    return torch.optim.AdamW(params, lr=f32(lr), betas=(B1, B2), eps=ADAM_EPS, weight_decay=f32(wd))


class Scaler:
    """torch.cuda.amp.GradScaler.update(), restated: backoff 0.5 and a reset tracker on a non-finite step; else the tracker
    counts and `growth_interval` clean steps in a row double the scale.  growth_interval <= 0: a static scale."""

    def __init__(self, scale, growth_interval):
        self.scale, self.tracker, self.interval, self.applied = float(scale), 0, growth_interval, 0

    def update(self, found_inf):
        if not found_inf:
            self.applied += 1
        if self.interval <= 0:
            return
        if found_inf:
            self.scale *= 0.5
            self.tracker = 0
        else:
            self.tracker += 1
            if self.tracker >= self.interval:
                self.scale *= 2.0
                self.tracker = 0


def spread_gradients(n, steps, seed):
    """unscaled f32 gradients whose per-element magnitudes are spread over 2^-20 .. 2^4"""
    g = _gen(seed)
    mag = torch.exp2(torch.rand(n, generator=g) * 24 - 20)
    return (torch.randn(steps, n, generator=g) * mag).float()


N_FLAT = 8 * 1031 + 3  # a partly filled last block of 256, not a multiple of 4

SEG_LEN, N_SEG = 8 * 129 + 4, 5
# segment ids with a gradient at each step, padded to n_active = 8 by repeating (the same segment several times in `active`).
# segment 2: never; segment 1: once (step 2), then idle — it keeps decaying with a zero gradient and its own step count
ACTIVITY = [[0], [0, 1], [0, 4], [0, 3], [3], [0, 4, 3], [0], [4], [0, 3], [0, 3, 4], [0], [0, 4]]
