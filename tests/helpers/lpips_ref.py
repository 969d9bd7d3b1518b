"""fp32 torch restatement of lpips 0.1.4 `LPIPS(net="vgg", version="0.1")` in eval mode: the oracle of the LPIPS tests.

Step by step as the package's published code runs it (lpips/lpips.py `LPIPS.forward`, `ScalingLayer`,
`normalize_tensor`, `spatial_average`; lpips/pretrained_networks.py `vgg16` over torchvision's `features[0:30]`):
scaling layer, the VGG16 convolutions (+ bias, ReLU) with 2x2 max-pools between stages, the five ReLU taps,
channel normalisation, the squared difference weighted by the 1x1 linear head (Dropout is the identity in eval), the
spatial mean, and the sum over layers.  The weights are synthetic and seeded (`synthetic_weights`): the real ones are
not available here, so parity is against the published algorithm, not against the package.
"""
import torch
import torch.nn.functional as F

SHIFT = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
SCALE = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256),
            (256, 512), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)  # the conv positions whose ReLU is tapped (relu1_2 .. relu5_3); a pool follows the first 4
TAP_CHANNELS = (64, 128, 256, 512, 512)


def synthetic_weights(seed: int = 0):
    """torchvision vgg16 `features` keys (He-normal, std sqrt(2 / fan_in), small biases) and lpips v0.1 linear heads
    (|N(0, 1)| / C) -> (vgg_state, lin_state)"""
    g = torch.Generator().manual_seed(seed)
    vgg = {}
    for i, (ci, co) in zip(CONV_INDEX, CHANNELS):
        vgg[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        vgg[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.01
    lin = {f"lin{k}.model.1.weight": torch.randn(1, c, 1, 1, generator=g).abs() / c for k, c in enumerate(TAP_CHANNELS)}
    return vgg, lin


def scaling_layer(x):
    return (x - SHIFT.to(x.device)) / SCALE.to(x.device)


def vgg_taps(x, vgg, n_stages: int = 5):
    """ReLU outputs relu1_2 .. relu{n_stages}_* of the scaled input"""
    taps, h = [], x
    for n, i in enumerate(CONV_INDEX):
        if len(taps) == n_stages:
            break
        h = F.relu(F.conv2d(h, vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"], padding=1))
        if n in TAP_AFTER:
            taps.append(h)
            if n != TAP_AFTER[-1]:
                h = F.max_pool2d(h, kernel_size=2, stride=2)
    return taps


def normalize_tensor(x, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm_factor + eps)


def layer_distances(in0, in1, vgg, lin, n_stages: int = 5):
    """[k] -> (B, 1, 1, 1) spatial mean of the weighted squared difference of tap k"""
    f0, f1 = vgg_taps(scaling_layer(in0), vgg, n_stages), vgg_taps(scaling_layer(in1), vgg, n_stages)
    out = []
    for k in range(len(f0)):
        diff = (normalize_tensor(f0[k]) - normalize_tensor(f1[k])) ** 2
        out.append(F.conv2d(diff, lin[f"lin{k}.model.1.weight"]).mean([2, 3], keepdim=True))
    return out


def lpips(in0, in1, vgg, lin, n_stages: int = 5):
    """LPIPS(in0, in1) for (B, 3, H, W) in [-1, 1] -> (B, 1, 1, 1)"""
    with torch.no_grad():
        res = layer_distances(in0.float(), in1.float(), vgg, lin, n_stages)
        val = res[0]
        for r in res[1:]:
            val = val + r
        return val


class Oracle:
    """the lpips.LPIPS call contract over the restatement (injected into the harness on the host)"""

    def __init__(self, vgg, lin):
        self.vgg, self.lin = vgg, lin

    def __call__(self, in0, in1):
        return lpips(in0.cpu(), in1.cpu(), self.vgg, self.lin)
