"""Fine-tuning a baked scene against pixels: the marcher's backward pass (`upnerf_baked_render_bwd`, csrc/baked.hip;
include/upnerf_hip.h states the gradient), an autograd function over it and a tuner round it.

    params = SceneParams.of(scene)                                      # fp32 leaves: rgbs, or (coef, sigma) of an SH scene
    out = render(params, rays, step=0.01)                               # {"rgb", "depth", "opacity"}: any torch loss works on them
    tuner = scene.tune(lr=1e-2)                                         # = BakedTuner(scene, 1e-2)
    loss = tuner.step(rays, target_rgb, step=0.01); tuned = tuner.scene()
    tuned, curve = distill(system, scene, [0, 3, 5], iters=200, batch=4096, baked_step=0.01, seed=0, img_id=3)

Dense scenes of degree 0, 1 and 2.  A sparse scene is refused: its pool stores the faces bricks share once per brick, so a
gradient would have to be summed over the copies -- `scene.densify()`, tune, `.sparsify()`, or baked_sparse_tune.py, which tunes
the pool in place and does that sum.  The occupancy is frozen while tuning:
a grid point whose sigma is zero is no parameter (it receives no gradient), so a clear cell keeps its eight zero corners, and a
sigma the optimiser drives to zero (`upnerf_baked_project`) is dead from then on.  A scene's environment (`scene.env`,
baked_env.py) is frozen too: the render composites it behind the march, the points see its gradient through the opacity
(g_opacity - g_rgb . env(d)), the map itself gets none.  The gradient's sums over rays are float atomic
adds: two runs agree to rounding, not to the bit.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import SIGMA_BYTE, BakedScene, Layout, _common, _rays16, _render_args, _upstream, a_scene, face_sum, march, pack_records, pack_rgbs
from .baked_env import composite_backward
from .baked_reg import tuner_tv
from .ops import TIMER
from .static_scene import require_cuda

__all__ = ["SceneParams", "render", "backward", "project", "BakedTuner", "distill", "SPARSE_REFUSAL"]

SPARSE_REFUSAL = ("a sparse baked scene cannot be tuned: its pool stores the faces that bricks share once per brick, so a gradient "
                  "would have to be summed over the copies -- tune scene.densify() and sparsify() the result")


def _dense(scene, what: str) -> None:
    if a_scene(scene, what).sparse:
        raise ValueError(SPARSE_REFUSAL)


def unpack_records(records: torch.Tensor, degree: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(coef fp32 [Nz, Ny, Nx, 3, nb], sigma fp32 [Nz, Ny, Nx]) of an SH scene's records: the stored halves converted exactly.
    (Any leading shape: the records of a pool [n_bricks, 9, 9, 9, 32 | 64] give [n_bricks, 9, 9, 9, 3, nb] and [n_bricks, 9, 9, 9].)"""
    nb = (degree + 1) ** 2
    coef = records[..., :6 * nb].contiguous().view(torch.float16).to(torch.float32).view(records.shape[:-1] + (3, nb))
    at = SIGMA_BYTE[degree]
    return coef.contiguous(), records[..., at:at + 4].contiguous().view(torch.float32).squeeze(-1).contiguous()


class Params:
    """The fp32 parameters of a scene over its points, grid or pool, with their `layout`: `rgbs` [.., 4] at degree 0, else `coef`
    [.., 3, nb] and `sigma` [..], where [..] is layout.shape.  The tensors are leaves a caller may set requires_grad on; `tensors`
    lists them.  SceneParams (dense, below) and baked_sparse_tune.PoolParams are its two constructors."""

    noun = "scene"  # what the refusal calls the points

    def __init__(self, layout: Layout, rgbs=None, coef=None, sigma=None, env=None):
        self.layout, self.occupancy, self.bounds, self.degree = layout, layout.occupancy, layout.bounds, layout.degree
        self.slots, self.bricks = layout.slots, layout.bricks
        self.rgbs, self.coef, self.sigma, self.env = rgbs, coef, sigma, env
        ok = self.degree in (0, 1, 2) and all(t is not None and t.dtype == torch.float32 and tuple(t.shape) == shape
                                              for t, shape in zip(self.tensors, layout.param_shapes))
        if not ok:
            raise ValueError(f"a degree-{self.degree} {self.noun} of {layout.shape} points has fp32 rgbs [.., 4] (degree 0) or "
                             f"coef [.., 3, nb] and sigma [..]")
        require_cuda(type(self).__name__, *((layout.slots, layout.bricks) if layout.sparse else ()), *self.tensors)

    @classmethod
    def _of(cls, scene: BakedScene, requires_grad: bool, *head) -> "Params":
        """The parameters of an accepted scene, a copy of its rgbs or its records unpacked: cls(*head, the tensors, the scene's env)."""
        if scene.sh_degree == 0:
            p = cls(*head, rgbs=scene.grid.detach().clone(), env=scene.env)
        else:
            coef, sigma = unpack_records(scene.grid, scene.sh_degree)
            p = cls(*head, coef=coef, sigma=sigma, env=scene.env)
        for t in p.tensors:
            t.requires_grad_(requires_grad)
        return p

    @property
    def tensors(self):
        return (self.rgbs,) if self.degree == 0 else (self.coef, self.sigma)


class SceneParams(Params):
    """The fp32 parameters of a dense scene with what the marcher needs beside them: `rgbs` [Nz, Ny, Nx, 4] at degree 0, else
    `coef` [Nz, Ny, Nx, 3, nb] and `sigma` [Nz, Ny, Nx]; the (frozen) occupancy, the bounds, the degree."""

    def __init__(self, occupancy, bounds, degree: int, rgbs=None, coef=None, sigma=None, env=None):
        super().__init__(Layout(occupancy, bounds, degree), rgbs, coef, sigma, env)

    @classmethod
    def of(cls, scene: BakedScene, requires_grad: bool = True) -> "SceneParams":
        _dense(scene, "SceneParams.of")
        return cls._of(scene, requires_grad, scene.occupancy, scene.bounds, scene.sh_degree)


def _forward(points: torch.Tensor, layout: Layout, rays, step, background, stop):
    R, dev = rays.shape[0], rays.device
    rgb, depth, opacity = torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    march(points, layout, rays, step, background, stop, rgb, depth, opacity)
    return rgb, depth, opacity


def _backward(what: str, points: torch.Tensor, layout: Layout, rays, step, background, stop, g_rgb, g_depth, g_opacity, out, sum_faces):
    """The marcher's backward pass on the points of `layout`, grid or pool: upnerf_baked_render_bwd or
    upnerf_baked_sparse_render_bwd, then on a pool with `sum_faces` the face sum over every gradient array.  The gradient is
    ADDED into `out` (zeroed here when None) and returned as `out` was given: one tensor at degree 0, else the pair."""
    require_cuda(what, points, rays, g_rgb)
    step, background, stop = _render_args(rays, step, background, stop)
    rays = _rays16(rays)
    R, degree = rays.shape[0], layout.degree
    _upstream(R, g_rgb, g_depth, g_opacity)
    if points.numel() * points.element_size() != math.prod(layout.shape) * layout.point_bytes:
        raise ValueError(f"points is the pool of {layout.shape[0]} bricks at degree {degree}" if layout.sparse else
                         f"points is the grid of {layout.shape} points at degree {degree}")
    if out is None:
        zeros = layout.zeros(rays.device)
        out = zeros if degree else zeros[0]
    outs = (out,) if degree == 0 else tuple(out)
    want = layout.param_shapes
    if len(outs) != len(want) or any(t.dtype != torch.float32 or tuple(t.shape) != w for t, w in zip(outs, want)):
        raise ValueError(f"out is fp32 {want}")
    grads = dict(grad=ptr(out)) if degree == 0 else dict(grad_coef=ptr(out[0]), grad_sigma=ptr(out[1]))
    address, slots = layout.pointers(points)
    upstream = dict(g_rgb=ptr(g_rgb.contiguous()), g_depth=ptr(g_depth.contiguous()) if g_depth is not None else None,
                    g_opacity=ptr(g_opacity.contiguous()) if g_opacity is not None else None)
    common = _common(layout.occupancy, layout.bounds, rays, step, background, stop)
    if layout.sparse:
        name, a = "baked_sparse_render_bwd", _lib.BakedSparseRenderBwdArgs(degree=degree, pool=address, slots=slots, **upstream, **grads, **common)
    else:
        name, a = "baked_render_bwd", _lib.BakedRenderBwdArgs(degree=degree, points=address, slots=None, **upstream, **grads, **common)
    fn = getattr(lib, "upnerf_" + name)
    check(TIMER.run(name, lambda: fn(C.byref(a), stream()), units=R), "upnerf_" + name)
    if layout.sparse and sum_faces:
        for t in outs:
            face_sum(t, layout)
    return out


def backward(points: torch.Tensor, degree: int, occupancy, bounds, rays: torch.Tensor, step: float, background: float, stop: float,
             g_rgb: torch.Tensor, g_depth: Optional[torch.Tensor] = None, g_opacity: Optional[torch.Tensor] = None, out=None):
    """upnerf_baked_render_bwd, called directly.  points: the grid the forward marched (`rgbs` [Nz, Ny, Nx, 4] fp32 at degree 0,
    the uint8 records at degree 1 | 2).  Returns the gradient ADDED into `out` (zeroed here when None): one fp32 tensor
    [Nz, Ny, Nx, 4] at degree 0, else the pair ([Nz, Ny, Nx, 3, nb], [Nz, Ny, Nx])."""
    return _backward("baked_tune.backward", points, Layout(occupancy, bounds, degree), rays, step, background, stop, g_rgb, g_depth,
                     g_opacity, out, False)


def project(degree: int, rgbs: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None) -> None:
    """upnerf_baked_project in place: `rgbs` [.., 4] at degree 0, `sigma` [..] at degree 1 | 2."""
    t = rgbs if degree == 0 else sigma
    n = t.numel() // 4 if degree == 0 else t.numel()
    a = _lib.BakedProjectArgs(n=n, degree=degree, rgbs=ptr(rgbs) if degree == 0 else None, sigma=ptr(sigma) if degree else None)
    check(TIMER.run("baked_project", lambda: lib.upnerf_baked_project(C.byref(a), stream()), units=n), "upnerf_baked_project")


class _Render(torch.autograd.Function):
    """The marcher with its backward (on a pool: and the face sum): (rgb, depth, opacity) of the parameter tensors of a Params."""

    @staticmethod
    def forward(ctx, params, rays, step, background, stop, *tensors):
        if params.degree == 0:
            points = tensors[0].detach().contiguous()
        else:  # the records the marcher reads; the gradient passes straight through the fp16 rounding to the fp32 coefficients
            points = pack_records(tensors[0].detach().contiguous(), tensors[1].detach().contiguous(), params.degree, 0.0)
        ctx.points, ctx.params, ctx.rays, ctx.args = points, params, rays, (step, background, stop)
        ctx.set_materialize_grads(False)
        return _forward(points, params.layout, rays, step, background, stop)

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_opacity):
        p, R = ctx.params, ctx.rays.shape[0]
        if g_rgb is None:
            g_rgb = torch.zeros(R, 3, device=ctx.rays.device)
        out = _backward("baked_tune.render", ctx.points, p.layout, ctx.rays, *ctx.args, g_rgb.contiguous(), g_depth, g_opacity, None, True)
        return (None,) * 5 + ((out,) if p.degree == 0 else tuple(out))


def _render(what: str, params: Params, rays: torch.Tensor, step: float, background: float, stop: float) -> dict:
    """render and baked_sparse_tune.render on parameters their caller has accepted."""
    require_cuda(what, rays)
    step, background, stop = _render_args(rays, step, background, stop)
    rays = _rays16(rays)
    rgb, depth, opacity = _Render.apply(params, rays, step, background if params.env is None else 0.0, stop, *params.tensors)
    if params.env is not None:
        rgb = params.env.composite(rays, rgb, opacity)
    return {"rgb": rgb, "depth": depth, "opacity": opacity}


def render(scene_params: SceneParams, rays: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0) -> dict:
    """{"rgb" [R, 3], "depth" [R], "opacity" [R]} of `rays` [R, 8] through the scene of `scene_params`, differentiable with
    respect to scene_params.rgbs, or to scene_params.coef and .sigma: forward the existing marcher (at degree 1 | 2 on records
    packed from the parameters by upnerf_baked_sh_pack at level 0), backward upnerf_baked_render_bwd.  No gradient for the rays.
    With scene_params.env set: the march at background 0 (`background` is not looked at), then the environment's composite through
    its own autograd function -- the points receive g_opacity - g_rgb . env(d) through the opacity."""
    if not isinstance(scene_params, SceneParams):
        raise ValueError("scene_params is a baked_tune.SceneParams (SceneParams.of(scene))")
    return _render("baked_tune.render", scene_params, rays, step, background, stop)


class BakedTuner:
    """Adam on the points of a dense scene against target pixels.  Holds the fp32 masters (one flat buffer: rgbs, or the
    coefficients followed by the sigmas), their gradient and the Adam moments; the occupancy is the scene's and is frozen.
    Everything that depends on the layout -- the shape of the point array, the forward and the gradient launches -- comes from
    self.layout, the scene's; baked_sparse_tune.PoolTuner is this tuner on a brick pool."""

    def __init__(self, scene: BakedScene, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 tv_sigma: float = 0.0, tv_colour: float = 0.0, tv_eps: float = 1e-8):
        self._accept(scene)
        lr, eps = float(lr), float(eps)
        if not (lr > 0 and np.isfinite(lr)) or not (eps > 0) or not all(0 <= float(b) < 1 for b in betas):
            raise ValueError("lr and eps are positive, the betas in [0, 1)")
        self.tv_sigma, self.tv_colour, self.tv_eps = float(tv_sigma), float(tv_colour), float(tv_eps)
        if not (np.isfinite(self.tv_sigma) and np.isfinite(self.tv_colour) and self.tv_eps > 0 and np.isfinite(self.tv_eps)):
            raise ValueError("tv_sigma and tv_colour are finite weights, tv_eps is positive and finite")
        self.lr, self.betas, self.eps, self.t = lr, (float(betas[0]), float(betas[1])), eps, 0
        self.layout = scene.layout
        self.degree, self.bounds, self.level, self.occupancy = scene.sh_degree, scene.bounds, scene.level, scene.occupancy
        self.env = scene.env  # frozen: composited behind the march in step(), carried to scene()
        # the total variation penalty (baked_reg): off at the defaults, and then nothing is launched for it
        self.last_tv = None
        self.tv_cells = max(1, self.occupancy.n_occupied()) if self.tv_on else None
        dev = scene.device
        shape, grid = self.layout.shape, scene.grid
        nb, n = (self.degree + 1) ** 2, math.prod(shape)
        per = 4 if self.degree == 0 else 3 * nb + 1
        self.p = torch.empty(n * per, device=dev)
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        view = lambda t: (t.view(shape + (4,)),) if self.degree == 0 else (t[:n * 3 * nb].view(shape + (3, nb)), t[n * 3 * nb:].view(shape))
        self.masters, self.grads = view(self.p), view(self.g)
        if self.degree == 0:
            self.masters[0].copy_(grid)
            self.records = None
        else:
            coef, sigma = unpack_records(grid, self.degree)
            self.masters[0].copy_(coef), self.masters[1].copy_(sigma)
            self.records = pack_records(*self.masters, self.degree, 0.0)

    def _accept(self, scene) -> None:
        _dense(scene, "BakedTuner")

    def _gradient(self, rays, step, background, stop, g_rgb, g_opacity=None) -> None:
        """The gradient of the points, added into self.grads (zeroed by the caller); with the penalty on, its gradient after the
        marcher's (upnerf_baked_tv), the value left in self.last_tv.  On a pool the face sum comes last, ONE over the per-copy
        gradients of both."""
        out = self.grads[0] if self.degree == 0 else self.grads
        _backward("BakedTuner.step", self.points, self.layout, rays, step, background, stop, g_rgb, None, g_opacity, out, not self.tv_on)
        if self.tv_on:
            self.last_tv = tuner_tv(self)
            if self.layout.sparse:
                for t in self.grads:
                    face_sum(t, self.layout)

    @property
    def tv_on(self) -> bool:
        return self.tv_sigma != 0.0 or self.tv_colour != 0.0

    def _settings(self) -> dict:
        return dict(betas=self.betas, eps=self.eps, tv_sigma=self.tv_sigma, tv_colour=self.tv_colour, tv_eps=self.tv_eps)

    @torch.no_grad()
    def upsampled(self) -> "BakedTuner":
        """A fresh tuner of the same kind and settings on self.scene().upsample(): twice the cells per axis, the Adam state
        reset (t = 0, zero moments)."""
        return type(self)(self.scene().upsample(), self.lr, **self._settings())

    @torch.no_grad()
    def pruned(self, rays: torch.Tensor, step: float, min_weight: Optional[float] = None, stop: float = 0.0) -> "BakedTuner":
        """A fresh tuner of the same kind and settings on self.scene().prune(rays, step, min_weight, stop) -- without the points
        that `rays` give less than `min_weight` (default: that no ray sees) -- the Adam state reset."""
        return type(self)(self.scene().prune(rays, step, min_weight, stop), self.lr, **self._settings())

    @property
    def points(self) -> torch.Tensor:
        """The grid the marcher reads now: the master rgbs, or the records packed from the masters."""
        return self.masters[0] if self.degree == 0 else self.records

    @property
    def nbytes(self) -> int:
        """Device bytes the tuner holds: masters, gradient, two moments, and at degree 1 | 2 the records."""
        return 4 * self.p.numel() * 4 + (self.records.numel() if self.records is not None else 0)

    @torch.no_grad()
    def step(self, rays: torch.Tensor, target_rgb: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0) -> torch.Tensor:
        """One iteration on `rays` [R, 8] against `target_rgb` [R, 3]: zero the gradient (upnerf_zero), forward, the gradient of
        the mean squared error (plain torch), upnerf_baked_render_bwd, with tv_sigma or tv_colour not zero upnerf_baked_tv,
        upnerf_adam, upnerf_baked_project, and at degree 1 | 2 upnerf_baked_sh_pack.  Returns the loss BEFORE the update, a 0-dim device tensor (no host read here).
        With an environment the march runs at background 0 (`background` is not looked at), upnerf_env_composite follows it, and
        upnerf_env_composite_bwd gives the marcher's backward its g_opacity = -(g_rgb . env(d))."""
        require_cuda("BakedTuner.step", rays, target_rgb)
        step, background, stop = _render_args(rays, step, background, stop)
        rays = _rays16(rays)
        R = rays.shape[0]
        if target_rgb.dtype != torch.float32 or tuple(target_rgb.shape) != (R, 3):
            raise ValueError("target_rgb is a fp32 tensor [R, 3]")
        st = stream()
        check(lib.upnerf_zero(ptr(self.g), self.g.numel(), st), "upnerf_zero")
        if self.env is not None:
            background = 0.0
        rgb, _, opacity = _forward(self.points, self.layout, rays, step, background, stop)
        if self.env is not None:
            self.env.composite_(rays, rgb, opacity)
        diff = rgb - target_rgb
        loss = (diff * diff).mean()
        g_rgb = diff * (2.0 / (3 * R))
        g_opacity = None
        if self.env is not None:
            g_opacity = composite_backward(self.env.env, rays, opacity, g_rgb)[0]
        self._gradient(rays, step, background, stop, g_rgb, g_opacity)
        self.t += 1
        b1, b2 = self.betas
        step_size, bc2_sqrt = self.lr / (1.0 - b1 ** self.t), math.sqrt(1.0 - b2 ** self.t)
        check(TIMER.run("adam", lambda: lib.upnerf_adam(self.p.numel(), ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), b1, b2,
                                                       self.eps, step_size, bc2_sqrt, None, st), units=self.p.numel()), "upnerf_adam")
        if self.degree == 0:
            project(0, rgbs=self.masters[0])
        else:
            project(self.degree, sigma=self.masters[1])
            pack_records(*self.masters, self.degree, 0.0, out=self.records)
        return loss

    def _pruned_points(self) -> torch.Tensor:
        """The masters pruned again at the scene's level: fresh rgbs (upnerf_baked_pack) or records (upnerf_baked_sh_pack)."""
        if self.degree:
            return pack_records(*self.masters, self.degree, self.level)
        rgbs = self.masters[0]
        return pack_rgbs(rgbs[..., 3].contiguous(), rgbs[..., :3].contiguous(), self.level)

    @torch.no_grad()
    def scene(self) -> BakedScene:
        """The tuned scene: the masters pruned again at the scene's level, the bits rebuilt."""
        return BakedScene.from_points(self._pruned_points(), self.bounds, self.level, self.degree).with_environment(self.env)


def keyframe_rays(path, device) -> torch.Tensor:
    """[K * W * H, 8] the rays of a path's own keyframe cameras, keyframe by keyframe (upnerf_path_rays)."""
    from .novel_view import path_poses, path_rays
    W, H = path.img_wh
    c2w, nf = path_poses(path.key_c2w.to(device), path.key_near_far.to(device), path.u.to(device), path.mode)  # (as render_path)
    return path_rays(c2w, nf, (W, H), path.K, 0, path.n_frames * W * H)[0]


def distill(system, scene: BakedScene, path_or_img_ids, iters: int, batch: int, baked_step: float, seed: int = 0, lr: float = 1e-2,
            img_id: Optional[int] = None, chunk: Optional[int] = None, tv: Tuple[float, float] = (0.0, 0.0), upsample_at: Sequence[int] = (),
            prune_at: Sequence[int] = (), prune_weight: Optional[float] = None):
    """Fit a dense baked scene to the field's own renders.  Cameras: the keyframes of a `novel_view.CameraPath`, or the refined
    training cameras `img_ids` (two at least).  The targets are rendered ONCE from the field by the static renderer
    (static_scene.render_static, through render_path) for those cameras' rays, all under the appearance of training image
    `img_id` -- the ONE appearance the scene was baked with.  Batches of `batch` rays are drawn with a generator seeded by `seed`;
    `iters` steps of BakedTuner(scene, lr) at sample spacing `baked_step`.  Returns (the tuned scene, the loss curve as a list of
    floats -- one host read, at the end).  tv = (tv_sigma, tv_colour): the tuner's total variation weights.  upsample_at: before
    each listed iteration (0-based) the tuner is replaced by tuner.upsampled() -- the returned scene has the final resolution; the
    sample spacing stays `baked_step`.  prune_at: before each listed iteration the tuner is replaced by tuner.pruned(all the cameras'
    rays, baked_step, prune_weight) -- what those rays give less than prune_weight (None: what none of them sees) leaves the scene
    (DESIGN.md 2.39); an iteration listed in both prunes first, then upsamples.  With prune_at empty nothing changes and nothing is
    launched."""
    _dense(scene, "distill")
    return _distill(BakedTuner, system, scene, path_or_img_ids, iters, batch, baked_step, seed, lr, img_id, chunk, tv, upsample_at,
                    prune_at, prune_weight)


def _distill(make_tuner, system, scene, path_or_img_ids, iters, batch, baked_step, seed, lr, img_id, chunk, tv=(0.0, 0.0), upsample_at=(),
             prune_at=(), prune_weight=None):
    """distill on a scene its caller has accepted, with the tuner make_tuner(scene, lr)."""
    from .novel_view import CameraPath, render_path
    if img_id is None:
        raise ValueError("img_id: the training image whose appearance the scene was baked with (the targets are rendered under it)")
    iters, batch = int(iters), int(batch)
    if iters < 1 or batch < 1:
        raise ValueError("iters and batch are positive")
    tv_sigma, tv_colour = (float(x) for x in tv)
    upsample_at = sorted(int(i) for i in upsample_at)
    if any(not 0 <= i < iters for i in upsample_at) or len(set(upsample_at)) != len(upsample_at):
        raise ValueError(f"upsample_at lists distinct iterations in [0, {iters})")
    prune_at = sorted(int(i) for i in prune_at)
    if any(not 0 <= i < iters for i in prune_at) or len(set(prune_at)) != len(prune_at):
        raise ValueError(f"prune_at lists distinct iterations in [0, {iters})")
    if prune_weight is not None and float(prune_weight) != float(prune_weight):
        raise ValueError("prune_weight is not a number")
    src = path_or_img_ids if isinstance(path_or_img_ids, CameraPath) else \
        CameraPath.through_images(system, list(path_or_img_ids), n_frames=len(list(path_or_img_ids)))
    K = src.key_c2w.shape[0]
    ids = torch.full((K,), int(img_id), dtype=torch.int32)
    keys = CameraPath(src.key_c2w, src.key_near_far, torch.arange(K, dtype=torch.float32), ids, ids, torch.zeros(K), src.img_wh, src.K, "linear")
    dev = scene.device
    target = render_path(system, keys, chunk=chunk, outputs=("rgb_float",))["rgb_float"].reshape(-1, 3).contiguous()
    rays = keyframe_rays(keys, dev)
    background = 1.0 if getattr(system.train_dataset, "white_back", False) else 0.0
    tuner = make_tuner(scene, lr, tv_sigma=tv_sigma, tv_colour=tv_colour) if tv_sigma or tv_colour else make_tuner(scene, lr)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    curve = []
    for it in range(iters):
        if it in prune_at:
            tuner = tuner.pruned(rays, baked_step, prune_weight)
        if it in upsample_at:
            tuner = tuner.upsampled()
        idx = torch.randint(0, rays.shape[0], (min(batch, rays.shape[0]),), generator=gen).to(dev)
        curve.append(tuner.step(rays[idx], target[idx], baked_step, background=background))
    return tuner.scene(), [float(x) for x in torch.stack(curve).cpu()]
