"""Image metrics of the novel-view-synthesis table (utils/metric.py of the reference): PSNR, SSIM and LPIPS of held-out
renders.

`ssim` / `ssim_rays` run the HIP kernel `upnerf_ssim` (csrc/metrics.hip): kornia's `ssim_loss` with a 3x3 window, as the
reference calls it, followed by the reference's `1 - 2 * dssim`, computed where the render already is -- no copy to the
host.  There is no CPU path: CPU tensors raise.  `psnr` is the reference's formula in torch ops.  LPIPS (AlexNet) is
`LpipsAlex` / `lpips_rays` of lpips.py, re-exported here: HIP as well, on weights the user supplies (no pretrained file is
part of this repository)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _image_ptr(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
    if t.dtype != torch.float32:
        raise TypeError(f"SSIM takes fp32 images (got {t.dtype})")
    return t.data_ptr()


def _ssim_launch(pred, gt, N, Ch, H, W, pred_stride, gt_stride, want_map: bool):
    """One upnerf_ssim call; strides are (n, c, y, x) in elements.  Returns (ssim [N], map [N, C, H, W] or None)."""
    if H < 2 or W < 2:
        raise ValueError(f"SSIM needs at least 2 x 2 pixels (reflect padding), got H={H}, W={W}")
    a = _lib.SsimArgs(N=N, C=Ch, H=H, W=W, pred=_image_ptr(pred), gt=_image_ptr(gt))
    a.pred_stride[:] = list(pred_stride)
    a.gt_stride[:] = list(gt_stride)
    n_scratch = _lib.lib.upnerf_ssim_scratch(C.byref(a))
    if n_scratch < 0:
        _lib.check(n_scratch, "upnerf_ssim_scratch")
    scratch = torch.empty(n_scratch, dtype=torch.float64, device=pred.device)
    out = torch.empty(N, dtype=torch.float32, device=pred.device)
    smap = torch.empty(N, Ch, H, W, dtype=torch.float32, device=pred.device) if want_map else None
    a.ssim, a.map = _lib.ptr(out), _lib.ptr(smap)
    _lib.check(_lib.lib.upnerf_ssim(C.byref(a), _lib.ptr(scratch), _lib.stream()), "upnerf_ssim")
    return out, smap


def ssim(image_pred: torch.Tensor, image_gt: torch.Tensor, reduction: str = "mean", window_size: int = 3) -> torch.Tensor:
    """utils/metric.py:23-30 on (N, C, H, W) images: "mean" -> 0-d tensor, the mean of the per-image SSIM;
    "none" -> the (N, C, H, W) map 1 - 2 * clamp((1 - s) / 2, 0, 1)."""
    if window_size != 3:
        raise ValueError("only the reference's 3 x 3 window is implemented")
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    if image_pred.dim() != 4 or image_pred.shape != image_gt.shape:
        raise ValueError(f"expected two (N, C, H, W) tensors of one shape, got {tuple(image_pred.shape)} and "
                         f"{tuple(image_gt.shape)}")
    N, Ch, H, W = image_pred.shape
    per_image, smap = _ssim_launch(image_pred, image_gt, N, Ch, H, W, image_pred.stride(), image_gt.stride(),
                                   want_map=reduction == "none")
    if reduction == "mean":
        return per_image.mean()
    return 1.0 - 2.0 * torch.clamp((1.0 - smap) / 2.0, 0.0, 1.0)


def parse_img_wh(img_wh) -> tuple:
    """(W, H) from the forms a validation batch carries it in: a collated [tensor([W]), tensor([H])], a tensor [2] or
    [1, 2], or two ints."""
    if torch.is_tensor(img_wh):
        vals = img_wh.reshape(-1).tolist()
    else:
        vals = [int(v.reshape(-1)[0]) if torch.is_tensor(v) else int(v) for v in img_wh]
    if len(vals) != 2:
        raise ValueError(f"img_wh must hold (W, H), got {img_wh!r}")
    return int(vals[0]), int(vals[1])


def ssim_rays(rgb: torch.Tensor, rgb_gt: torch.Tensor, img_wh) -> torch.Tensor:
    """SSIM of renders in the ray layout ([H*W, 3] or [N, H*W, 3], ray y*W + x is pixel (y, x)): per-image values [N]."""
    W, H = parse_img_wh(img_wh)
    p = rgb if rgb.dim() == 3 else rgb[None]
    g = rgb_gt if rgb_gt.dim() == 3 else rgb_gt[None]
    if p.dim() != 3 or p.shape != g.shape:
        raise ValueError(f"expected [H*W, C] or [N, H*W, C] renders of one shape, got {tuple(rgb.shape)} and "
                         f"{tuple(rgb_gt.shape)}")
    N, R, Ch = p.shape
    if W * H != R:
        raise ValueError(f"img_wh = ({W}, {H}) does not match {R} rays")
    st = lambda t: (t.stride(0), t.stride(2), W * t.stride(1), t.stride(1))
    return _ssim_launch(p, g, N, Ch, H, W, st(p), st(g), want_map=False)[0]


def psnr(image_pred: torch.Tensor, image_gt: torch.Tensor, valid_mask=None, reduction: str = "mean") -> torch.Tensor:
    """utils/metric.py:10-20."""
    value = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == "mean":
        value = torch.mean(value)
    return -10 * torch.log10(value)


from .lpips import LpipsAlex, lpips_rays  # noqa: E402,F401  (lpips.py takes parse_img_wh from this module when called)
