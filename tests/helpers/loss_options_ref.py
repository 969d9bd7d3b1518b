"""float64 restatement of the two training-objective options, written from the published
algorithms; torch only, no GPU.

Min-SNR-gamma weighting (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy"; the `compute_snr`
function and the `snr_gamma` block of diffusers' examples/text_to_image/train_text_to_image.py):

    snr(t) = alphas_cumprod[t] / (1 - alphas_cumprod[t])
    epsilon:       w(t) = min(snr, gamma) / snr
    v_prediction:  w(t) = min(snr, gamma) / (snr + 1)
    loss = mean_b( w(t_b) * mean_chw( (pred_b - target_b)^2 ) )

Offset noise (the `noise_offset` line of the same script):

    noise' = noise + s * xi[:, :, None, None],   xi ~ N(0, 1) of shape (B, C)

The inputs keep the values they have (an f32 alphas_cumprod table is read as the f32 numbers it holds); the arithmetic is
float64."""
import torch


def scaled_linear_alphas_cumprod_f32(num_train=1000, beta_start=0.00085, beta_end=0.012):
    """the f32 table the engine holds: DDPMScheduler(beta_schedule="scaled_linear") computed in float32"""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def snr(ac, t):
    a = ac.double()[torch.as_tensor(t, dtype=torch.int64)]
    return a / (1.0 - a)


def min_snr_weight(ac, t, gamma, v_prediction=False):
    """float64 weights of the timesteps t (any shape); gamma may be inf"""
    s = snr(ac, t)
    clipped = torch.minimum(s, torch.full_like(s, float(gamma)))
    return clipped / (s + 1.0 if v_prediction else s)


def offset_noise(noise, xi, s):
    """noise (B, C, H, W) + s * xi (B, C) broadcast over the pixels, float64"""
    return noise.double() + float(s) * xi.double()[:, :, None, None]


def add_noise(latents, noise, ac, t, v_prediction):
    """DDPMScheduler.add_noise / get_velocity in float64 -> (noisy, target)"""
    a = ac.double()[torch.as_tensor(t, dtype=torch.int64)].view(-1, 1, 1, 1)
    sa, sb = a.sqrt(), (1.0 - a).sqrt()
    z, n = latents.double(), noise.double()
    return sa * z + sb * n, (sa * n - sb * z) if v_prediction else n


def weighted_mse(pred, target, w):
    """(loss, dloss/dpred) in float64: loss = mean_b(w_b mean_chw(d^2)), gradient 2 d w_b / N; pred, target (B, C, H, W)"""
    d = pred.double() - target.double()
    wb = w.double().view(-1, 1, 1, 1)
    return (wb * d * d).mean(), 2.0 * d * wb / d.numel()
