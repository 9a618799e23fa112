"""fp64 restatement of the reference's SSIM (utils/metric.py:23-30: kornia 0.6/0.7 ssim_loss(img1, img2, window_size=3,
max_val=1, eps=1e-12, reduction=..., padding="same"), then 1 - 2 * dssim) in torch CPU ops: reflect padding + a grouped
conv2d with the normalised 3x3 Gaussian window, moments as kornia forms them (filter(x^2) - mu^2).  Not kornia itself,
which the test machines do not have; the CPU tests check it against an independent restatement and closed forms."""
import math

import torch
import torch.nn.functional as F

C1, C2, EPS = 1e-4, 9e-4, 1e-12


def window(dtype=torch.float64):
    g = torch.tensor([math.exp(-(x * x) / (2 * 1.5 ** 2)) for x in (-1, 0, 1)], dtype=dtype)
    g = g / g.sum()
    return torch.outer(g, g)


def _filter(x, pad_mode="reflect"):
    """kornia filter2d(border_type="reflect") with the 3x3 window on (N, C, H, W)."""
    C = x.shape[1]
    k = window(x.dtype)[None, None].expand(C, 1, 3, 3)
    if pad_mode == "zeros":
        xp = F.pad(x, (1, 1, 1, 1))
    else:
        xp = F.pad(x, (1, 1, 1, 1), mode=pad_mode)
    return F.conv2d(xp, k, groups=C)


def ssim_map(img1, img2, pad_mode="reflect"):
    """The raw per-pixel s (kornia's ssim_map) in fp64, (N, C, H, W)."""
    x, y = img1.double(), img2.double()
    mu1, mu2 = _filter(x, pad_mode), _filter(y, pad_mode)
    s11 = _filter(x * x, pad_mode) - mu1 * mu1
    s22 = _filter(y * y, pad_mode) - mu2 * mu2
    s12 = _filter(x * y, pad_mode) - mu1 * mu2
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2)
    return num / (den + EPS)


def ssim_per_image(img1, img2, pad_mode="reflect"):
    """1 - 2 * mean over (c, y, x) of clamp((1 - s) / 2, 0, 1), one value per image, fp64."""
    loss = torch.clamp((1 - ssim_map(img1, img2, pad_mode)) / 2, 0, 1)
    return 1 - 2 * loss.flatten(1).mean(1)


def rays_to_nchw(rgb, W, H):
    """[H*W, C] or [N, H*W, C] (ray y*W + x is pixel (y, x)) -> (N, C, H, W)."""
    r = rgb if rgb.dim() == 3 else rgb[None]
    return r.reshape(r.shape[0], H, W, r.shape[2]).permute(0, 3, 1, 2)
