"""Posing a photograph against a baked scene: the marcher's gradient with respect to the rays (`upnerf_baked_ray_bwd`,
csrc/baked.hip; include/upnerf_hip.h states the gradient), an autograd function over it and a localiser round it.

    g_rays = ray_backward(scene, rays, step, background, stop, g_rgb)     # [R, 8]: the gradient of o | d | near | far
    out = render(scene, rays, step=0.01)                                 # {"rgb", "depth", "opacity"}, differentiable in `rays`
    loc = BakedLocaliser(scene, targets, K, c2w_init, near_far, lr=1e-2)
    loss = loc.step(batch=4096, baked_step=0.01, generator=gen); poses = loc.poses()
    poses, curve = localise(scene, targets, K, c2w_init, near_far, iters=200, batch=4096, baked_step=0.01)

Dense and sparse scenes of degree 0, 1 and 2; the scene is constant (baked_tune.py and baked_sparse_tune.py differentiate the
points and give the rays no gradient).  The gradient is that of the piecewise-smooth function the marcher computes: the samples a
ray visits and the cell of each are held fixed.  Every ray's row is written by its own thread: the same bits every run.  The
chain to se(3) is camera.refine_and_get_rays' (upnerf_pose_rays_fwd / _bwd).  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import BakedScene, _common, _rays16, _render_args, _upstream, a_scene
from .ops import TIMER
from .static_scene import require_cuda

__all__ = ["ray_backward", "render", "BakedLocaliser", "localise", "pixel_directions"]


def ray_backward(scene: BakedScene, rays: torch.Tensor, step: float, background: float, stop: float, g_rgb: torch.Tensor,
                 g_depth: Optional[torch.Tensor] = None, g_opacity: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """upnerf_baked_ray_bwd, called directly: the gradient [R, 8] of a loss with the upstream gradients g_rgb [R, 3], g_depth
    [R] | None and g_opacity [R] | None with respect to the rows of `rays` [R, 8], WRITTEN into `out` (allocated when None)."""
    a_scene(scene, "baked_pose.ray_backward")
    require_cuda("baked_pose.ray_backward", rays, g_rgb)
    step, background, stop = _render_args(rays, step, background, stop)
    rays = _rays16(rays)
    R, dev = rays.shape[0], rays.device
    _upstream(R, g_rgb, g_depth, g_opacity)
    if out is None:
        out = torch.empty(R, 8, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (R, 8) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out is a contiguous fp32 tensor [R, 8] on the rays' device")
    g_rgb = g_rgb.contiguous()  # (kept alive until the launch is enqueued)
    g_depth = g_depth.contiguous() if g_depth is not None else None
    g_opacity = g_opacity.contiguous() if g_opacity is not None else None
    points, slots = scene.layout.pointers(scene.points)
    a = _lib.BakedRayBwdArgs(degree=scene.sh_degree, points=points, slots=slots, g_rgb=ptr(g_rgb), g_depth=ptr(g_depth),
                             g_opacity=ptr(g_opacity), g_rays=ptr(out), **_common(scene.occupancy, scene.bounds, rays, step, background, stop))
    check(TIMER.run("baked_ray_bwd", lambda: lib.upnerf_baked_ray_bwd(C.byref(a), stream()), units=R), "upnerf_baked_ray_bwd")
    return out


class _Render(torch.autograd.Function):
    """The marcher with its ray gradient: (rgb, depth, opacity) of the rays; the scene is constant."""

    @staticmethod
    def forward(ctx, scene, rays, step, background, stop):
        ctx.scene, ctx.rays, ctx.args = scene, _rays16(rays), (step, background, stop)
        ctx.set_materialize_grads(False)
        out = scene.render(ctx.rays, step, background, stop)
        return out["rgb"], out["depth"], out["opacity"]

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_opacity):
        R = ctx.rays.shape[0]
        if g_rgb is None:
            g_rgb = torch.zeros(R, 3, device=ctx.rays.device)
        return None, ray_backward(ctx.scene, ctx.rays, *ctx.args, g_rgb.contiguous(), g_depth, g_opacity), None, None, None


def render(scene: BakedScene, rays: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0) -> dict:
    """{"rgb" [R, 3], "depth" [R], "opacity" [R]} of `rays` [R, 8] through `scene`, differentiable with respect to `rays` only:
    forward the marcher of the scene's layout and degree (BakedScene.render, the same bits), backward upnerf_baked_ray_bwd.
    With scene.env set: the march at background 0 (`background` is not looked at), then the environment's composite through its
    own autograd function (upnerf_env_composite / _bwd) -- the rays receive the gradient of both, the sky's included."""
    a_scene(scene, "baked_pose.render")
    require_cuda("baked_pose.render", rays)
    step, background, stop = _render_args(rays, step, background, stop)
    if scene.env is None:
        rgb, depth, opacity = _Render.apply(scene, rays, step, background, stop)
    else:
        rgb, depth, opacity = _Render.apply(scene.with_environment(None), rays, step, 0.0, stop)
        rgb = scene.env.composite(rays, rgb, opacity)
    return {"rgb": rgb, "depth": depth, "opacity": opacity}


def pixel_directions(x: torch.Tensor, y: torch.Tensor, K) -> torch.Tensor:
    """[n, 3] camera-space directions of the pixels (x, y) of a camera K = (fx, fy, cx, cy): ((x - cx) / fx, -(y - cy) / fy, -1),
    on the integer pixel grid as upnerf_path_rays forms them."""
    fx, fy, cx, cy = (float(k) for k in K)
    x, y = x.to(torch.float32), y.to(torch.float32)
    return torch.stack([(x - cx) / fx, -(y - cy) / fy, -torch.ones_like(x)], 1)


class BakedLocaliser:
    """Registers N >= 1 photographs against a baked scene: Adam on an se(3) row per photograph, composed on to `c2w_init` by
    camera.refine_and_get_rays.  targets [N, H, W, 3] fp32 on the device, K = (fx, fy, cx, cy), c2w_init [N, 3, 4], near_far a
    pair or [N, 2].  Holds se3 [N, 6], zero at first."""

    def __init__(self, scene: BakedScene, targets: torch.Tensor, K, c2w_init: torch.Tensor, near_far, lr: float = 1e-2,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, background: float = 0.0, stop: float = 0.0):
        a_scene(scene, "BakedLocaliser")
        require_cuda("BakedLocaliser", targets, c2w_init)
        if targets.dtype != torch.float32 or targets.dim() != 4 or targets.shape[3] != 3 or targets.shape[0] < 1:
            raise ValueError("targets is a fp32 tensor [N, H, W, 3] with N >= 1")
        N, H, W = (int(n) for n in targets.shape[:3])
        if c2w_init.dtype != torch.float32 or tuple(c2w_init.shape) != (N, 3, 4):
            raise ValueError("c2w_init is a fp32 tensor [N, 3, 4], one pose per target")
        lr, eps = float(lr), float(eps)
        if not (lr > 0 and np.isfinite(lr)) or not (eps > 0) or not all(0 <= float(b) < 1 for b in betas) or len(tuple(K)) != 4:
            raise ValueError("lr and eps are positive, the betas in [0, 1), K is (fx, fy, cx, cy)")
        dev = targets.device
        nf = torch.as_tensor(near_far, dtype=torch.float32).to(dev)
        self.near_far = (nf[None].expand(N, 2) if nf.dim() == 1 else nf).contiguous()
        if tuple(self.near_far.shape) != (N, 2):
            raise ValueError("near_far is a pair or [N, 2]")
        self.scene, self.K, self.N, self.H, self.W = scene, tuple(float(k) for k in K), N, H, W
        self.background, self.stop = float(background), float(stop)
        self.targets = targets.reshape(N * H * W, 3).contiguous()
        self.c2w_init = c2w_init.contiguous()
        self.se3 = torch.zeros(N, 6, device=dev, requires_grad=True)
        self.opt = torch.optim.Adam([self.se3], lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps)  # (6 N numbers: not hot)

    def rays_of(self, idx: torch.Tensor) -> torch.Tensor:
        """[n, 8] the rays of the pixels `idx` of the virtual list [N][H][W] under the poses as they are now; differentiable
        with respect to self.se3."""
        from .camera import refine_and_get_rays
        img, pix = idx // (self.H * self.W), idx % (self.H * self.W)
        dirs = pixel_directions(pix % self.W, pix // self.W, self.K)
        o, d = refine_and_get_rays(self.se3[img], self.c2w_init[img], dirs)
        return torch.cat([o, d, self.near_far[img]], 1)

    def step(self, batch: int, baked_step: float, generator: torch.Generator) -> torch.Tensor:
        """One iteration: `batch` pixels drawn over all images with `generator` (a CPU generator), their rays under the poses
        as they are, baked_pose.render, the mean squared error of the colours, backward through upnerf_baked_ray_bwd and
        upnerf_pose_rays_bwd, Adam.  Returns the loss BEFORE the update, a 0-dim device tensor (no host read here)."""
        n = self.N * self.H * self.W
        idx = torch.randint(0, n, (min(int(batch), n),), generator=generator).to(self.se3.device)
        self.opt.zero_grad(set_to_none=True)
        out = render(self.scene, self.rays_of(idx), baked_step, self.background, self.stop)
        diff = out["rgb"] - self.targets[idx]
        loss = (diff * diff).mean()
        loss.backward()
        self.opt.step()
        return loss.detach()

    @torch.no_grad()
    def poses(self) -> torch.Tensor:
        """[N, 3, 4] the refined poses (pose_align.refined_poses: the HIP pose kernel)."""
        from .pose_align import refined_poses
        return refined_poses(self.se3.detach(), self.c2w_init)


def localise(scene: BakedScene, targets: torch.Tensor, K, c2w_init: torch.Tensor, near_far, iters: int, batch: int, baked_step: float,
             seed: int = 0, lr: float = 1e-2, background: float = 0.0, stop: float = 0.0):
    """`iters` steps of BakedLocaliser on batches drawn with a generator seeded by `seed`.  Returns (the refined poses
    [N, 3, 4], the loss curve as a list of floats -- one host read, at the end)."""
    iters, batch = int(iters), int(batch)
    if iters < 1 or batch < 1:
        raise ValueError("iters and batch are positive")
    loc = BakedLocaliser(scene, targets, K, c2w_init, near_far, lr=lr, background=background, stop=stop)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    curve = [loc.step(batch, baked_step, gen) for _ in range(iters)]
    return loc.poses(), [float(x) for x in torch.stack(curve).cpu()]
