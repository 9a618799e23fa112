"""What lies outside the box of a baked scene: a direction-only environment, a cube map of the colour the field shows from the box
outwards, composited behind the march with the transmittance that is left (csrc/env.hip; include/upnerf_hip.h states the map, the
lookup and the gradient).

    env = Environment.build(system, bounds, E=64, img_id=3)             # 6 (E+1)^2 node rays through the field, then the seam pass
    scene = scene.with_environment(env)                                 # or BakedScene.build(..., env_size=64)
    out = scene.render(rays, step=0.01)                                 # the march with background 0, then env.composite
    rgb = env.composite(rays, rgb, opacity)                             # differentiable in rgb, opacity and rays
    colours = env.lookup(dirs)

Compositing is linear -- rgb = rgb_marched(background = 0) + (1 - opacity) env(d) -- so the marcher and its backward kernels are
the ones they were; with no environment nothing here is launched.  The map is baked from the field and stays FROZEN: the tuners
give it no gradient.  It has NO PARALLAX: it is what the field shows from the box CENTRE between the box and `far`, and is exact
only for a camera there; from elsewhere far content sits at infinity.  How close that comes to the field on a trained scene is
unchecked.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import _appearance
from .ops import TIMER
from .static_scene import box, c_float3, require_cuda

__all__ = ["Environment", "node_rays", "seam", "composite_backward"]


def _size(E) -> int:
    if int(E) != E or not 1 <= int(E) <= _lib.ENV_MAX_E:
        raise ValueError(f"E is the number of cells per face side, 1 .. {_lib.ENV_MAX_E}, got {E!r}")
    return int(E)


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """The contiguous fp32 tensor `t` itself where its address is a multiple of 16, else a copy at such an address."""
    t = t.contiguous()
    if t.data_ptr() % 16 == 0:
        return t
    spare = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    off = (-spare.data_ptr() % 16) // 4
    return spare[off:off + t.numel()].view(t.shape).copy_(t)


def node_rays(bounds, E: int, far: float, n0: int, count: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[count, 8] the ray rows o | d | near | far of nodes n0 .. n0 + count of an E-cell map round the box `bounds`
    (upnerf_env_rays): from the box centre along the node's unit direction, near where the ray leaves the box."""
    lo, hi = box(bounds, strict=True)
    E = _size(E)
    if out is None:
        out = torch.empty(count, 8, device=device, dtype=torch.float32)
    a = _lib.EnvRaysArgs(E=E, count=int(count), n0=int(n0), lo=c_float3(lo), hi=c_float3(hi), far=float(far), rays=ptr(out))
    check(TIMER.run("env_rays", lambda: lib.upnerf_env_rays(C.byref(a), stream()), units=int(count)), "upnerf_env_rays")
    return out[:count]


def seam(env: torch.Tensor) -> torch.Tensor:
    """upnerf_env_seam in place on a map [6, E+1, E+1, 4]: every copy of a shared node takes the bytes of the copy on the lowest
    face.  Returns `env`."""
    E = env.shape[1] - 1
    a = _lib.EnvSeamArgs(E=E, env=ptr(env))
    check(TIMER.run("env_seam", lambda: lib.upnerf_env_seam(C.byref(a), stream()), units=24 * E), "upnerf_env_seam")
    return env


def composite_backward(env: torch.Tensor, rays: torch.Tensor, opacity: torch.Tensor, g_out: torch.Tensor):
    """upnerf_env_composite_bwd, called directly: (g_opacity [R], g_rays [R, 8]) of the upstream gradient g_out [R, 3]."""
    R = rays.shape[0]
    g_opacity, g_rays = torch.empty(R, device=rays.device), torch.empty(R, 8, device=rays.device)
    g_out = g_out.contiguous()
    a = _lib.EnvCompositeBwdArgs(E=env.shape[1] - 1, R=R, env=ptr(env), rays=ptr(rays), opacity=ptr(opacity), g_out=ptr(g_out),
                                 g_opacity=ptr(g_opacity), g_rays=ptr(g_rays))
    check(TIMER.run("env_composite_bwd", lambda: lib.upnerf_env_composite_bwd(C.byref(a), stream()), units=R), "upnerf_env_composite_bwd")
    return g_opacity, g_rays


def _composite(env: torch.Tensor, rays: torch.Tensor, opacity: torch.Tensor, rgb: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    R = rays.shape[0]
    a = _lib.EnvCompositeArgs(E=env.shape[1] - 1, R=R, env=ptr(env), rays=ptr(rays), opacity=ptr(opacity), rgb_in=ptr(rgb), rgb_out=ptr(out))
    check(TIMER.run("env_composite", lambda: lib.upnerf_env_composite(C.byref(a), stream()), units=R), "upnerf_env_composite")
    return out


class _Composite(torch.autograd.Function):
    """rgb_out of (rays, rgb, opacity); the map is constant."""

    @staticmethod
    def forward(ctx, env, rays, rgb, opacity):
        rays, opacity = _aligned16(rays.detach()), opacity.detach().contiguous()
        ctx.env, ctx.rays, ctx.opacity = env, rays, opacity
        rgb = rgb.detach().contiguous()
        return _composite(env, rays, opacity, rgb, torch.empty_like(rgb))

    @staticmethod
    def backward(ctx, g_out):
        need_rays, need_rgb, need_opacity = ctx.needs_input_grad[1:4]
        g_opacity = g_rays = None
        if need_rays or need_opacity:
            g_opacity, g_rays = composite_backward(ctx.env, ctx.rays, ctx.opacity, g_out)
        return None, g_rays if need_rays else None, g_out if need_rgb else None, g_opacity if need_opacity else None


class Environment:
    """`env` [6, E+1, E+1, 4] fp32 on the device, 16-byte aligned: r, g, b and a zero at the corner nodes of the six faces (the
    layout of include/upnerf_hip.h)."""

    def __init__(self, env: torch.Tensor):
        require_cuda("Environment", env)
        if env.dtype != torch.float32 or env.dim() != 4 or env.shape[0] != 6 or env.shape[1] != env.shape[2] or env.shape[3] != 4 or \
                env.shape[1] < 2 or env.shape[1] - 1 > _lib.ENV_MAX_E:
            raise ValueError(f"an environment is a fp32 tensor [6, E+1, E+1, 4] with 1 <= E <= {_lib.ENV_MAX_E}")
        self.env = _aligned16(env.detach())

    @classmethod
    def from_array(cls, env, device="cuda") -> "Environment":
        """From a map of the caller's own: a tensor or array [6, E+1, E+1, 4] (the fourth float is padding) or [6, E+1, E+1, 3]
        (padded here).  The caller keeps the copies of shared nodes equal (`seam` does), or the lookup has seams."""
        t = torch.as_tensor(env) if not torch.is_tensor(env) else env
        t = t.detach().to(torch.float32)
        if t.dim() == 4 and t.shape[3] == 3:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], 3)
        if not t.is_cuda:
            t = t.to(device)
        return cls(t.contiguous().clone())

    @classmethod
    @torch.no_grad()
    def build(cls, system, bounds, E: int, far: Optional[float] = None, img_id=None, rows=None, field: str = "fine") -> "Environment":
        """Bake the environment of the box `bounds`: the static colour (sched_mult = 1) that render_static gives the 6 (E+1)^2 node
        rays of upnerf_env_rays -- from the box centre, from where they leave the box to `far` (default: the largest far plane of
        the training images) -- under the appearance of training image `img_id` (or `rows`, a row of the caller's own: the
        arguments of BakedScene.build), val.chunk_size rays at a time, then upnerf_env_seam.  `field` names the network whose
        appearance table the row is checked against and whose colour is taken."""
        from .static_scene import field_of, near_far, render_static, static_keys
        model, dev = field_of(system, field, "Environment.build")
        E = _size(E)
        lo, hi = box(bounds, strict=True)
        if far is None:
            far = max(near_far(system, i)[1] for i in range(system.se3_refine.weight.shape[0]))
        far = float(far)
        if not (far > 0 and np.isfinite(far)):
            raise ValueError(f"far is a positive, finite distance, got {far}")
        keys = static_keys(system, 1)
        row = {k: _appearance(system, system.models[f"nerf_{k[:-2]}"], k[:-2], img_id, rows, dev) for k in keys}
        N = 6 * (E + 1) ** 2
        chunk = min(int(system.hparams["val.chunk_size"]), N)
        env = torch.zeros(N, 4, device=dev, dtype=torch.float32)
        rays_ws = torch.empty(chunk, 8, device=dev, dtype=torch.float32)
        rows_ws = {k: r.expand(chunk, -1).contiguous() for k, r in row.items() if r is not None}
        for n0 in range(0, N, chunk):
            n = min(chunk, N - n0)
            rays = node_rays((lo, hi), E, far, n0, n, dev, out=rays_ws)
            res = render_static(system, rays, {k: r[:n] for k, r in rows_ws.items()}, 1)
            env[n0:n0 + n, :3].copy_(res[f"s_rgb_{field}"])
        return cls(seam(_aligned16(env.view(6, E + 1, E + 1, 4))))

    # ---- use -----------------------------------------------------------------------------------------------------------------

    def lookup(self, dirs: torch.Tensor) -> torch.Tensor:
        """[n, 3] env(d) of the directions `dirs` [n, 3] (never normalised; a row that is not finite or all zero gives zeros):
        upnerf_env_composite on rays with these directions, opacity 0 and a black picture."""
        require_cuda("Environment.lookup", dirs)
        if dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[1] != 3:
            raise ValueError("dirs are a fp32 tensor [n, 3]")
        n = dirs.shape[0]
        rays = torch.zeros(n, 8, device=dirs.device)
        rays[:, 3:6] = dirs.detach()
        out = torch.zeros(n, 3, device=dirs.device)
        return _composite(self.env, rays, torch.zeros(n, device=dirs.device), out, out)

    def composite(self, rays: torch.Tensor, rgb: torch.Tensor, opacity: torch.Tensor) -> torch.Tensor:
        """[R, 3] rgb + (1 - opacity) env(d) for rays [R, 8] (upnerf_env_composite): `rgb` [R, 3] and `opacity` [R] of a march with
        background 0.  Differentiable in `rgb`, `opacity` and `rays` (upnerf_env_composite_bwd; face and cell held fixed); the
        map gets no gradient."""
        require_cuda("Environment.composite", rays, rgb, opacity)
        R = rays.shape[0] if rays.dim() == 2 else -1
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError("rays are a fp32 tensor [R, 8] (o | d | near | far)")
        if rgb.dtype != torch.float32 or tuple(rgb.shape) != (R, 3) or opacity.dtype != torch.float32 or tuple(opacity.shape) != (R,):
            raise ValueError("rgb is a fp32 tensor [R, 3] and opacity a fp32 tensor [R]")
        return _Composite.apply(self.env, rays, rgb, opacity)

    def composite_(self, rays: torch.Tensor, rgb: torch.Tensor, opacity: torch.Tensor) -> torch.Tensor:
        """composite in place on `rgb` [>= R, 3] (contiguous; rays 16-byte aligned), no autograd: what BakedScene.render calls."""
        return _composite(self.env, rays, opacity, rgb, rgb)

    # ---- accessors -------------------------------------------------------------------------------------------------------------

    @property
    def E(self) -> int:
        return self.env.shape[1] - 1

    @property
    def device(self):
        return self.env.device

    @property
    def nbytes(self) -> int:
        return self.env.numel() * 4
