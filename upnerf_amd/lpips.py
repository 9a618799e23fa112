"""LPIPS (AlexNet) of held-out renders from weights the user supplies: the third column of the reference's novel-view table
(models/nerf_system_optmize.py:184, `lpips_alex(img_gt, img)` on [0, 1] images with normalize=False).

The arithmetic runs in HIP where the render already is (csrc/lpips.hip: `upnerf_conv2d` on the fp32-input MFMA,
`upnerf_maxpool2d`, `upnerf_lpips_dist`); there is no CPU path and no pretrained file in this repository.  The user has the
two files: torchvision's AlexNet checkpoint and the lpips package's `alex.pth`; `LpipsAlex.load` reads them.  The network
and the key names below are written from the published lpips 0.1.x / torchvision sources and have not been compared with
the packages' own output (neither is installed where this was written)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .ops import TIMER

# (key prefix in torchvision's alexnet state_dict, C_out, C_in, k, stride, pad); a tap follows each convolution's ReLU
CONVS = (("features.0", 64, 3, 11, 4, 2), ("features.3", 192, 64, 5, 1, 2), ("features.6", 384, 192, 3, 1, 1),
         ("features.8", 256, 384, 3, 1, 1), ("features.10", 256, 256, 3, 1, 1))
# keys of the 1 x 1 "lin" layers in the lpips package's alex.pth, each [1, C, 1, 1] without a bias
LINS = tuple(f"lin{i}.model.1.weight" for i in range(5))
POOL_BEFORE = (False, True, True, False, False)  # a 3 x 3 stride-2 max pool in front of conv1 and conv2
MIN_SIDE = 31  # below this the last three taps have no pixel


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class LpipsAlex:
    """Five (weight, bias) pairs and five lin vectors as fp32 tensors, plus scratch per (N, H, W).  A plain object, not an
    nn.Module: attached to a NeRFSystemOptimize as `lpips_model` it stays out of the system's state_dict."""

    def __init__(self, convs, lins):
        convs, lins = list(convs), list(lins)
        if len(convs) != 5 or len(lins) != 5:
            raise ValueError("LpipsAlex takes five (weight, bias) pairs and five lin vectors")
        self.convs, self.lins = [], []
        for (key, co, ci, k, _, _), (w, b), lin_key, lin in zip(CONVS, convs, LINS, lins):
            if tuple(w.shape) != (co, ci, k, k):
                raise ValueError(f"{key}.weight: expected shape {(co, ci, k, k)}, got {tuple(w.shape)}")
            if tuple(b.shape) != (co,):
                raise ValueError(f"{key}.bias: expected shape {(co,)}, got {tuple(b.shape)}")
            if lin.numel() != co or tuple(lin.shape) not in ((co,), (1, co, 1, 1)):
                raise ValueError(f"{lin_key}: expected shape {(1, co, 1, 1)}, got {tuple(lin.shape)}")
            f = lambda t: t.detach().to(torch.float32).contiguous()
            self.convs.append((f(w), f(b)))
            self.lins.append(f(lin.reshape(co)))
        self._scratch = {}

    @classmethod
    def from_state_dicts(cls, alexnet_sd, lin_sd):
        """torchvision's `features.{0,3,6,8,10}.{weight,bias}` (classifier.* is ignored) and the lpips package's
        `lin{0..4}.model.1.weight`."""
        def get(sd, key):
            if key not in sd:
                raise ValueError(f"missing key {key!r}")
            return sd[key]
        convs = [(get(alexnet_sd, f"{c[0]}.weight"), get(alexnet_sd, f"{c[0]}.bias")) for c in CONVS]
        return cls(convs, [get(lin_sd, k) for k in LINS])

    @classmethod
    def load(cls, alexnet_path, lin_path):
        return cls.from_state_dicts(torch.load(alexnet_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True))

    def to(self, device):
        self.convs = [(w.to(device), b.to(device)) for w, b in self.convs]
        self.lins = [v.to(device) for v in self.lins]
        self._scratch = {}
        return self

    def cuda(self):
        return self.to("cuda")

    def scratch(self, N, H, W, device):
        """(activation buffer 0, activation buffer 1, fp64 partials) for N pairs of H x W images, kept for the next call."""
        key = (N, H, W, str(device))
        if key not in self._scratch:
            a = _lib.LpipsScratchArgs(N=N, H=H, W=W)
            _lib.check(_lib.lib.upnerf_lpips_scratch(C.byref(a)), "upnerf_lpips_scratch")
            self._scratch[key] = (torch.empty(a.act0_elems, dtype=torch.float32, device=device),
                                  torch.empty(a.act1_elems, dtype=torch.float32, device=device),
                                  torch.empty(a.part_elems, dtype=torch.float64, device=device))
        return self._scratch[key]

    def _run(self, x, N, H, W, stride, out=None):
        """x: the 2N images (renders, then targets) read through `stride` = (n, c, y, x) in elements.  Returns out [N]."""
        if self.convs[0][0].device != x.device:
            raise RuntimeError(f"LpipsAlex weights are on {self.convs[0][0].device}, the images on {x.device}; call .to()")
        bufs = self.scratch(N, H, W, x.device)
        part = bufs[2]
        if out is None:
            out = torch.empty(N, dtype=torch.float32, device=x.device)
        st = _lib.stream()
        cur, cur_buf = x, None  # cur_buf: which activation buffer holds `cur` (None: the caller's images)
        h, w, ch = H, W, 3
        for i, ((_, co, ci, k, s, p), (wt, b), lin) in enumerate(zip(CONVS, self.convs, self.lins)):
            if POOL_BEFORE[i]:
                dst = bufs[1 - cur_buf]
                a = _lib.Maxpool2dArgs(N=2 * N, C=ch, H=h, W=w, x=_lib.ptr(cur), y=_lib.ptr(dst))
                _lib.check(TIMER.run(f"lpips_pool{i}", lambda: _lib.lib.upnerf_maxpool2d(C.byref(a), st)), "upnerf_maxpool2d")
                h, w = _out(h, 3, 2, 0), _out(w, 3, 2, 0)
                cur, cur_buf = dst, 1 - cur_buf
                stride = (ch * h * w, h * w, w, 1)
            dst_buf = 0 if cur_buf is None else 1 - cur_buf
            dst = bufs[dst_buf]
            a = _lib.Conv2dArgs(N=2 * N, C_in=ci, H=h, W=w, C_out=co, k=k, stride=s, pad=p, relu=1, scale_in=int(i == 0),
                                x=cur.data_ptr(), w=_lib.ptr(wt), bias=_lib.ptr(b), y=_lib.ptr(dst))
            a.x_stride[:] = list(stride)
            h, w, ch = _out(h, k, s, p), _out(w, k, s, p), co
            _lib.check(TIMER.run(f"lpips_conv{i}", lambda: _lib.lib.upnerf_conv2d(C.byref(a), st),
                                 units=2 * co * ci * k * k * 2 * N * h * w), "upnerf_conv2d")  # (units: FLOP)
            cur, cur_buf = dst, dst_buf
            stride = (ch * h * w, h * w, w, 1)
            d = _lib.LpipsDistArgs(N=N, C=ch, H=h, W=w, accumulate=int(i > 0), feat=_lib.ptr(cur), w=_lib.ptr(lin),
                                   out=_lib.ptr(out))
            _lib.check(TIMER.run(f"lpips_dist{i}", lambda: _lib.lib.upnerf_lpips_dist(C.byref(d), _lib.ptr(part), st)),
                       "upnerf_lpips_dist")
        return out

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor, out=None) -> torch.Tensor:
        """LPIPS of (N, 3, H, W) images against their targets: [N].  Symmetric in its arguments."""
        if pred.dim() != 4 or pred.shape != gt.shape:
            raise ValueError(f"expected two (N, 3, H, W) tensors of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        N, Ch, H, W = pred.shape
        _check_images(pred, gt, Ch, H, W)
        x = torch.cat([pred, gt], 0)  # one batch of 2N: both sides see the same kernels, so model(x, x) == 0 exactly
        return self._run(x, N, H, W, x.stride(), out)


def _check_images(pred, gt, Ch, H, W):
    for t in (pred, gt):
        if not t.is_cuda:
            raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
        if t.dtype != torch.float32:
            raise TypeError(f"LPIPS takes fp32 images (got {t.dtype})")
    if Ch != 3:
        raise ValueError(f"LPIPS takes RGB images, got {Ch} channels")
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"LPIPS (AlexNet) needs at least {MIN_SIDE} x {MIN_SIDE} pixels, got H={H}, W={W}")


def lpips_rays(model: LpipsAlex, rgb: torch.Tensor, rgb_gt: torch.Tensor, img_wh) -> torch.Tensor:
    """LPIPS of renders in the ray layout ([H*W, 3] or [N, H*W, 3], ray y*W + x is pixel (y, x)): per-image values [N]."""
    from .metrics import parse_img_wh  # (metrics re-exports this module's names)
    W, H = parse_img_wh(img_wh)
    p = rgb if rgb.dim() == 3 else rgb[None]
    g = rgb_gt if rgb_gt.dim() == 3 else rgb_gt[None]
    if p.dim() != 3 or p.shape != g.shape:
        raise ValueError(f"expected [H*W, 3] or [N, H*W, 3] renders of one shape, got {tuple(rgb.shape)} and "
                         f"{tuple(rgb_gt.shape)}")
    N, R, Ch = p.shape
    if W * H != R:
        raise ValueError(f"img_wh = ({W}, {H}) does not match {R} rays")
    _check_images(p, g, Ch, H, W)
    x = torch.cat([p, g], 0)  # [2N, H*W, 3], read in place through its strides
    return model._run(x, N, H, W, (x.stride(0), x.stride(2), W * x.stride(1), x.stride(1)))
