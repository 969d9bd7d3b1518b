"""Loud 1-D parameters for the engine parity tests.

`view_neti_amd/synth.py` (`make_tensor`) draws every 1-D tensor almost trivially: a tensor named `*.bias` (Linear / conv
biases and norm shifts alike) is 0.02 * u, any other 1-D tensor (a norm gain) is 1 + 0.02 * u, u uniform in [-1, 1).  An
engine that drops, mis-indexes or swaps such an operand then moves the end result by less than the end-to-end bars
(tests/test_engine_taps_cpu.py keeps the count).  `loud` overrides that rule, and only that rule:

    `*.bias`            0.25 * N(0, 1)
    other 1-D tensors   1 + 0.5 * U(-1, 1)

drawn from ONE torch.Generator seeded with `seed`, in the dict's own order, then rounded to f16 (like every weight the
tests hand to both the engine and the oracle).  Tensors of two or more dimensions are passed through untouched (the same
objects).  Pure: the argument is not modified, and the same (dict, seed) gives the same bits.

These are the amplitudes the work started from; neither the CPU proof (tests/test_engine_taps_cpu.py: weakest margin 18 x a
bar) nor the GPU measurement (tests/helpers/engine_taps.py: every tap finite and within 1.5e-3 of the fp32 oracle, so no
f16 range problem) asked for others.  `drop` and `roll` are the two mutations of that proof.
"""
import torch

BIAS_STD = 0.25
GAIN_HALF_WIDTH = 0.5


def loud(state_dict, seed):
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, t in state_dict.items():
        if t.dim() != 1:
            out[name] = t
            continue
        if name.endswith(".bias"):
            v = BIAS_STD * torch.randn(t.shape, generator=gen)
        else:
            v = 1.0 + GAIN_HALF_WIDTH * (2.0 * torch.rand(t.shape, generator=gen) - 1.0)
        out[name] = v.half().float().to(t.device)
    return out


def names_1d(state_dict):
    return [k for k, t in state_dict.items() if t.dim() == 1]


def drop(state_dict, name):
    """what an engine computes that leaves the operand out: zeros for a `.bias`, ones for a gain"""
    t = state_dict[name]
    return dict(state_dict, **{name: torch.zeros_like(t) if name.endswith(".bias") else torch.ones_like(t)})


def roll(state_dict, name):
    """what an engine computes that reads the operand one element off"""
    return dict(state_dict, **{name: torch.roll(state_dict[name], 1)})
