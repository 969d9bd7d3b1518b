"""The exponential moving average of the mappers restated in float64: the decay of diffusers'
`EMAModel.get_decay` with inv_gamma = 1 and min_decay = 0, and one update.  Pure numpy, no GPU, nothing from the library."""
import numpy as np


def decay(k, max_decay, update_after_step=0, power=0.0):
    """the decay of the k-th applied update (k = 1, 2, ...): s = max(0, k - update_after_step - 1); 0 when s == 0, else
    (1 + s) / (10 + s) when power == 0, else 1 - (1 + s)^(-power); capped by max_decay.  All in float64."""
    s = max(0, int(k) - int(update_after_step) - 1)
    if s == 0:
        return 0.0
    s = np.float64(s)
    d = (1.0 + s) / (10.0 + s) if power == 0 else 1.0 - np.power(1.0 + s, -np.float64(power))
    return float(min(d, np.float64(max_decay)))


def update(e, p, c):
    """e + c * (p - e) in float64, c = 1 - decay (s_param.sub_(one_minus_decay * (s_param - param)))"""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + np.float64(c) * (p - e)


def f32(x):
    """x as the device holds it in an f32 hyper-parameter slot"""
    return float(np.float32(x))
