"""Restatement of guidance rescale (Lin, Liu, Li & Yang 2023, "Common Diffusion Noise Schedules and Sample Steps are
Flawed", section 3.4) as diffusers' `rescale_noise_cfg` evaluates it after classifier-free guidance, and of the
data-prediction sampler step that follows it.  Written from the published algorithm; torch only, no GPU.  `dtype` picks the
arithmetic: float64 is the reference, float32 on the CPU is the `ref32` of helpers.checks.check32.

    e     = u + g (c - u)                                              per sample b, over its (Lc, HW) elements:
    f[b]  = phi std(c[b]) / std(e[b]) + (1 - phi)                      (centred; the N - 1 of both cancels)
    e'    = f[b] e
    x0    = (x - sigma_t e') / alpha_t  (epsilon)  |  alpha_t x - sigma_t e'  (v_prediction)
    x    <- cx x + c0 x0 + c1 m_prev [+ cn noise],   m_prev <- x0

One deviation from diffusers: a prediction whose centred sum of squares is 0 (a constant e[b]) gets f[b] = 1 where
`rescale_noise_cfg` divides by zero.
"""
import torch


def unpack(pred, B, Lc, HW, dtype=torch.float64):
    """NHWC [2 B HW][ld] 16-bit UNet output -> (uncond, cond), each [B][Lc][HW] of the stored values"""
    p = pred[:, :Lc].to(dtype).cpu().view(2, B, HW, Lc).permute(0, 1, 3, 2)
    return p[0].contiguous(), p[1].contiguous()


def guided(u, c, guidance, dtype=torch.float64):
    u, c = u.to(dtype), c.to(dtype)
    return u + guidance * (c - u)


def _centred_ss(v):
    d = v - v.mean(dim=(1, 2), keepdim=True)
    return (d * d).sum(dim=(1, 2))


def rescale_factor(u, c, guidance, phi, dtype=torch.float64):
    """f[b] of the module docstring for u, c of shape [B][Lc][HW]"""
    c = c.to(dtype)
    e = guided(u, c, guidance, dtype)
    ss_c, ss_e = _centred_ss(c), _centred_ss(e)
    ratio = (ss_c / torch.where(ss_e > 0, ss_e, torch.ones_like(ss_e))).sqrt()
    return torch.where(ss_e > 0, phi * ratio + (1 - phi), torch.ones_like(ratio))


def sampler_step(x, e, m_prev, row, noise, v_prediction, factor=None, dtype=torch.float64):
    """one step on the guided prediction e (scaled by factor[b] when given); row = (alpha_t, sigma_t, cx, c0, c1, cn) ->
    (x_new, x0)"""
    x, e, m_prev = x.to(dtype), e.to(dtype), m_prev.to(dtype)
    a_t, s_t, cx, c0, c1, cn = row
    if factor is not None:
        e = factor.to(dtype).view(-1, 1, 1) * e
    x0 = a_t * x - s_t * e if v_prediction else (x - s_t * e) / a_t
    xn = cx * x + c0 * x0 + c1 * m_prev
    if noise is not None and cn != 0:
        xn = xn + cn * noise.to(dtype)
    return xn, x0
