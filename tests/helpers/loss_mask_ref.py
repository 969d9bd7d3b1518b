"""float64 restatement of the object-masked diffusion loss; torch only, no GPU.

Weights of one sample from a uint8 mask of H x W pixels, factor f, threshold thr, background weight bg:

    cnt_p  = #{pixels of latent cell p with value >= thr}                 (integers)
    m_p    = bg + (1 - bg) cnt_p / f^2
    norm   = sum_p m_p = bg h w + (1 - bg) (sum_p cnt_p) / f^2            (from the exact integer sum)
    q_p    = m_p (h w / norm),   a row of zeros where norm == 0

Loss, gradient and the per-sample form, with the optional Min-SNR weight w_b of helpers/loss_options_ref.py:

    loss   = sum_{b,c,p} w_b q_bp d^2 / N,   N = B C HW;       dloss/dpred = 2 d w_b q_bp / N
    out[b] = sum_{c,p} q_bp d^2 / (C HW)

so loss = mean_b[ w_b sum_{c,p} m d^2 / (C sum_p m) ]: every sample is normalised by its own mask mass.  The inputs keep the
values they have (bg is read as the f32 number the ABI is handed); the arithmetic is float64."""
import torch


def random_mask(H, W, seed, p=0.5):
    """uint8 (H, W) with values on both sides of the threshold 3: 0, 1, 2 are background, 3, 128, 255 foreground, drawn per
    pixel — almost every latent cell is partial"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0, 1, 2, 3, 128, 255], dtype=torch.uint8)
    fg = torch.rand(H, W, generator=g) < p
    pick = torch.randint(0, 3, (H, W), generator=g)
    return torch.where(fg, vals[3 + pick], vals[pick])


def blocky_mask(H, W, f, seed):
    """uint8 (H, W): whole cells of foreground (255) or background (0) at random, and one row of cells that are partial"""
    g = torch.Generator().manual_seed(seed)
    cells = (torch.rand(H // f, W // f, generator=g) < 0.5).to(torch.uint8) * 255
    m = cells.repeat_interleave(f, 0).repeat_interleave(f, 1).contiguous()
    row = (H // f) // 2
    m[row * f:(row + 1) * f] = random_mask(f, W, seed + 1)
    return m


def cell_counts(mask_u8, f, threshold=3):
    """integer counts per latent cell, (H/f, W/f) int64; mask_u8 (H, W) uint8"""
    H, W = mask_u8.shape
    assert H % f == 0 and W % f == 0
    fg = (mask_u8.to(torch.int64) >= int(threshold)).to(torch.int64)
    return fg.view(H // f, f, W // f, f).sum(dim=(1, 3))


def weights_from_mask(mask_u8, f, threshold=3, background=0.0):
    """float64 weights (h*w,) of one sample"""
    cnt = cell_counts(mask_u8, f, threshold).reshape(-1)
    hw, f2 = cnt.numel(), float(f * f)
    bg = float(torch.tensor(background, dtype=torch.float32))
    m = bg + (1.0 - bg) * (cnt.double() / f2)
    norm = bg * hw + (1.0 - bg) * (float(int(cnt.sum())) / f2)
    if not norm > 0.0:
        return torch.zeros(hw, dtype=torch.float64)
    return m * (hw / norm)


def weighted_loss(pred, target, q, w=None):
    """(loss, dloss/dpred) in float64; pred, target (B, C, HW), q (B, HW), w (B,) or None"""
    d = pred.double() - target.double()
    wq = q.double().unsqueeze(1)
    if w is not None:
        wq = wq * w.double().view(-1, 1, 1)
    return (wq * d * d).sum() / d.numel(), 2.0 * d * wq / d.numel()


def per_sample(pred, target, q):
    """float64 (B,): sum_{c,p} q_bp d^2 / (C HW)"""
    d = pred.double() - target.double()
    return (q.double().unsqueeze(1) * d * d).sum(dim=(1, 2)) / (d.shape[1] * d.shape[2])
