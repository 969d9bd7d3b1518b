"""float64 restatement of the DDIM update with eta (Song, Meng & Ermon, "Denoising Diffusion Implicit Models", eq. 12 and
16), in the order diffusers' DDIMScheduler.step evaluates it with set_alpha_to_one=False, clip_sample=False and
use_clipped_model_output=False (the Stable Diffusion scheduler configs), plus the classifier-free-guidance combination
that precedes it in sd_pipeline_call.  Written from the published algorithm; torch only, no GPU.

    a_t = alphas_cumprod[t],  a_prev = alphas_cumprod[t - T // N]  (alphas_cumprod[0] below timestep 0)
    epsilon:       x0 = (x - sqrt(1 - a_t) out)/sqrt(a_t),           eps = out
    v_prediction:  x0 = sqrt(a_t) x - sqrt(1 - a_t) out,             eps = sqrt(a_t) out + sqrt(1 - a_t) x
    variance = (1 - a_prev)/(1 - a_t) (1 - a_t/a_prev),  std = eta sqrt(variance)
    x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - std^2) eps + std noise
"""
import torch


def scaled_linear_alphas_cumprod(num_train=1000, beta_start=0.00085, beta_end=0.012):
    """the SD `scaled_linear` schedule: betas = linspace(sqrt(b0), sqrt(b1), T)^2, alphas_cumprod = cumprod(1 - betas)"""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, 0)


def ddim_timesteps(num_steps, num_train=1000):
    """DDIMScheduler.set_timesteps with steps_offset = 1: (arange(N) * (T // N)) reversed, + 1"""
    ratio = num_train // num_steps
    return [i * ratio + 1 for i in range(num_steps)][::-1]


def guided(uncond, cond, guidance):
    u, c = uncond.double(), cond.double()
    return u + guidance * (c - u)


def ddim_step(ac, t, prev_t, x, model_out, eta, noise, v_prediction):
    """one DDIMScheduler.step in float64; returns (x_prev, x0)"""
    ac, x, out = ac.double(), x.double(), model_out.double()
    a_t = ac[t]
    a_prev = ac[prev_t] if prev_t >= 0 else ac[0]
    b_t = 1 - a_t
    if v_prediction:
        x0 = a_t.sqrt() * x - b_t.sqrt() * out
        eps = a_t.sqrt() * out + b_t.sqrt() * x
    else:
        x0 = (x - b_t.sqrt() * out) / a_t.sqrt()
        eps = out
    variance = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
    std = eta * variance.sqrt()
    direction = (1 - a_prev - std ** 2).sqrt() * eps
    x_prev = a_prev.sqrt() * x0 + direction
    if eta > 0:
        x_prev = x_prev + std * noise.double()
    return x_prev, x0
