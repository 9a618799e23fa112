"""Fine-tuning a SPARSE baked scene in place, on its brick pool: the marcher's backward pass through the pool
(`upnerf_baked_sparse_render_bwd`, csrc/baked.hip) and the sum over the copies of the points that bricks share
(`upnerf_brick_face_sum`, csrc/brick.hip); include/upnerf_hip.h states both; DESIGN.md 2.35.  The sibling of baked_tune.py, whose
helpers, tuner loop and distill it uses:

    params = PoolParams.of(sparse_scene)                                # fp32 leaves over the pool: rgbs, or (coef, sigma)
    out = render(params, rays, step=0.01)                               # {"rgb", "depth", "opacity"}, differentiable
    tuner = sparse_scene.tune_pool(lr=1e-2)                             # = PoolTuner(sparse_scene, 1e-2)
    loss = tuner.step(rays, target_rgb, step=0.01); tuned = tuner.scene()
    tuned, curve = distill(system, sparse_scene, [0, 3, 5], iters=200, batch=4096, baked_step=0.01, seed=0, img_id=3)

Nothing is ever as large as the grid: masters, gradient and Adam moments are over the n_bricks * 729 points of the pool.  The
brick table is frozen, as the occupancy is in the dense tuner: a brick that is empty stays empty, and a brick whose points all
die stays in the pool as a zero brick (`scene.densify().sparsify()` compacts it).  A grid point on a face that bricks share is
stored once per brick.  The backward kernel gives each copy what the samples inside its own brick give it; the face sum then
writes the sum over the copies, formed in ascending brick order, to every copy -- so every copy sees the same gradient, and
copies that start with the same bytes (the layout's invariant) keep the same bytes through Adam, the projection and the packing.
A dense scene is refused: that is baked_tune's.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import POINT_BYTES, BakedScene, _common, _rays16, _render_args, march, pack_records
from .baked_tune import BakedTuner, _distill, unpack_records
from .ops import TIMER
from .static_scene import require_cuda

__all__ = ["PoolParams", "render", "backward", "face_sum", "PoolTuner", "distill", "DENSE_REFUSAL"]

DENSE_REFUSAL = ("a dense baked scene has no brick pool to tune: use baked_tune (scene.tune), or scene.sparsify() first")


def _sparse(scene, what: str) -> None:
    if not isinstance(scene, BakedScene):
        raise ValueError(f"{what} takes a baked.BakedScene")
    if not scene.sparse:
        raise ValueError(DENSE_REFUSAL)
    if scene.n_bricks < 1:
        raise ValueError(f"{what}: the scene has no occupied brick, so nothing to tune")


class PoolParams:
    """The fp32 parameters of a sparse scene over its pool, with what the marcher needs beside them: `rgbs`
    [n_bricks, 9, 9, 9, 4] at degree 0, else `coef` [n_bricks, 9, 9, 9, 3, nb] and `sigma` [n_bricks, 9, 9, 9]; the (frozen) table
    `slots` and `bricks`, the (frozen) occupancy, the bounds, the degree.  The tensors are leaves; `tensors` lists them."""

    def __init__(self, slots, bricks, occupancy, bounds, degree: int, rgbs=None, coef=None, sigma=None, env=None):
        self.slots, self.bricks, self.occupancy, self.bounds, self.degree = slots, bricks, occupancy, bounds, int(degree)
        self.rgbs, self.coef, self.sigma, self.env = rgbs, coef, sigma, env
        P, nb = _lib.BRICK_POINTS, (self.degree + 1) ** 2
        shape = (bricks.numel(), P, P, P)
        if self.degree == 0:
            ok = rgbs is not None and rgbs.dtype == torch.float32 and tuple(rgbs.shape) == shape + (4,)
        else:
            ok = self.degree in (1, 2) and coef is not None and sigma is not None and coef.dtype == sigma.dtype == torch.float32 and \
                tuple(coef.shape) == shape + (3, nb) and tuple(sigma.shape) == shape
        if not ok:
            raise ValueError(f"a degree-{degree} pool of {shape} points has fp32 rgbs [.., 4] (degree 0) or coef [.., 3, nb] and sigma [..]")
        require_cuda("PoolParams", slots, bricks, *self.tensors)

    @classmethod
    def of(cls, scene: BakedScene, requires_grad: bool = True) -> "PoolParams":
        _sparse(scene, "PoolParams.of")
        if scene.sh_degree == 0:
            p = cls(scene.slots, scene.bricks, scene.occupancy, scene.bounds, 0, rgbs=scene.pool.detach().clone(), env=scene.env)
        else:
            coef, sigma = unpack_records(scene.pool, scene.sh_degree)
            p = cls(scene.slots, scene.bricks, scene.occupancy, scene.bounds, scene.sh_degree, coef=coef, sigma=sigma, env=scene.env)
        for t in p.tensors:
            t.requires_grad_(requires_grad)
        return p

    @property
    def tensors(self):
        return (self.rgbs,) if self.degree == 0 else (self.coef, self.sigma)


def _table(layout):
    """(slots, bricks, (Cx, Cy, Cz)) of a sparse BakedScene or a PoolParams."""
    if isinstance(layout, BakedScene):
        _sparse(layout, "a pool's table")
    elif not isinstance(layout, PoolParams):
        raise ValueError("the layout is a sparse baked.BakedScene or a PoolParams")
    return layout.slots, layout.bricks, layout.occupancy.dims


def face_sum(t: torch.Tensor, scene) -> torch.Tensor:
    """upnerf_brick_face_sum in place on the pool-shaped fp32 tensor `t` [n_bricks, 9, 9, 9, ...] (any trailing shape: F floats per
    point) of `scene` (a sparse BakedScene or a PoolParams): every copy of a grid point that bricks share becomes the sum over
    its copies, in ascending brick order.  Returns `t`."""
    slots, bricks, (Cx, Cy, Cz) = _table(scene)
    require_cuda("baked_sparse_tune.face_sum", t)
    P, n = _lib.BRICK_POINTS, bricks.numel()
    if t.dtype != torch.float32 or t.dim() < 4 or tuple(t.shape[:4]) != (n, P, P, P) or not t.is_contiguous():
        raise ValueError(f"a pool-shaped tensor is contiguous fp32 [{n}, {P}, {P}, {P}, ...]")
    F = t.numel() // (n * P ** 3)
    a = _lib.BrickFaceSumArgs(Cx=Cx, Cy=Cy, Cz=Cz, n_bricks=n, F=F, slots=ptr(slots), bricks=ptr(bricks), data=ptr(t))
    check(TIMER.run("brick_face_sum", lambda: lib.upnerf_brick_face_sum(C.byref(a), stream()), units=n * 386 * F), "upnerf_brick_face_sum")
    return t


_sum_faces = face_sum  # (backward has an argument of that name)


def _forward(points: torch.Tensor, params: PoolParams, rays, step, background, stop):
    R, dev = rays.shape[0], rays.device
    rgb, depth, opacity = torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    march(points, params.degree, params.slots, params.occupancy, params.bounds, rays, step, background, stop, rgb, depth, opacity)
    return rgb, depth, opacity


def backward(points: torch.Tensor, params: PoolParams, rays: torch.Tensor, step: float, background: float, stop: float,
             g_rgb: torch.Tensor, g_depth: Optional[torch.Tensor] = None, g_opacity: Optional[torch.Tensor] = None, out=None,
             face_sum: bool = True):
    """upnerf_baked_sparse_render_bwd, called directly.  points: the pool the forward marched ([n_bricks, 9, 9, 9, 4] fp32 at
    degree 0, the uint8 records at degree 1 | 2); params: the table, occupancy, bounds and degree (its tensors are not read).
    Returns the gradient ADDED into `out` (zeroed here when None): one fp32 tensor [n_bricks, 9, 9, 9, 4] at degree 0, else the
    pair ([n_bricks, 9, 9, 9, 3, nb], [n_bricks, 9, 9, 9]).  face_sum = False leaves the raw per-copy gradient: each copy of a
    shared point holds what the samples inside its own brick gave it.  (With `out` given and face_sum = True the sum runs over
    what `out` holds afterwards, the caller's part included.)"""
    if not isinstance(params, PoolParams):
        raise ValueError("params is a baked_sparse_tune.PoolParams (PoolParams.of(scene))")
    require_cuda("baked_sparse_tune.backward", points, rays, g_rgb)
    step, background, stop = _render_args(rays, step, background, stop)
    rays = _rays16(rays)
    R, dev, degree = rays.shape[0], rays.device, params.degree
    if g_rgb.dtype != torch.float32 or tuple(g_rgb.shape) != (R, 3):
        raise ValueError("g_rgb is a fp32 tensor [R, 3]")
    for g in (g_depth, g_opacity):
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (R,)):
            raise ValueError("g_depth and g_opacity are fp32 tensors [R] or None")
    P, nb = _lib.BRICK_POINTS, (degree + 1) ** 2
    shape = (params.bricks.numel(), P, P, P)
    if points.numel() * points.element_size() != shape[0] * P ** 3 * POINT_BYTES[degree]:
        raise ValueError(f"points is the pool of {shape[0]} bricks at degree {degree}")
    if out is None:
        out = torch.zeros(shape + (4,), device=dev) if degree == 0 else (torch.zeros(shape + (3, nb), device=dev), torch.zeros(shape, device=dev))
    outs = (out,) if degree == 0 else tuple(out)
    want = (shape + (4,),) if degree == 0 else (shape + (3, nb), shape)
    if len(outs) != len(want) or any(t.dtype != torch.float32 or tuple(t.shape) != w for t, w in zip(outs, want)):
        raise ValueError(f"out is fp32 {want}")
    grads = dict(grad=ptr(out)) if degree == 0 else dict(grad_coef=ptr(out[0]), grad_sigma=ptr(out[1]))
    a = _lib.BakedSparseRenderBwdArgs(degree=degree, pool=ptr(points), slots=ptr(params.slots), g_rgb=ptr(g_rgb.contiguous()),
                                      g_depth=ptr(g_depth.contiguous()) if g_depth is not None else None,
                                      g_opacity=ptr(g_opacity.contiguous()) if g_opacity is not None else None, **grads,
                                      **_common(params.occupancy, params.bounds, rays, step, background, stop))
    check(TIMER.run("baked_sparse_render_bwd", lambda: lib.upnerf_baked_sparse_render_bwd(C.byref(a), stream()), units=R),
          "upnerf_baked_sparse_render_bwd")
    if face_sum:
        for t in outs:
            _sum_faces(t, params)
    return out


class _Render(torch.autograd.Function):
    """The sparse marcher with its backward and the face sum: (rgb, depth, opacity) of the parameter tensors of a PoolParams."""

    @staticmethod
    def forward(ctx, params, rays, step, background, stop, *tensors):
        if params.degree == 0:
            points = tensors[0].detach().contiguous()
        else:  # the records the marcher reads; the gradient passes straight through the fp16 rounding, as in baked_tune
            points = pack_records(tensors[0].detach().contiguous(), tensors[1].detach().contiguous(), params.degree, 0.0)
        ctx.points, ctx.params, ctx.rays, ctx.args = points, params, rays, (step, background, stop)
        ctx.set_materialize_grads(False)
        return _forward(points, params, rays, step, background, stop)

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_opacity):
        p, R = ctx.params, ctx.rays.shape[0]
        if g_rgb is None:
            g_rgb = torch.zeros(R, 3, device=ctx.rays.device)
        out = backward(ctx.points, p, ctx.rays, *ctx.args, g_rgb.contiguous(), g_depth, g_opacity)
        return (None,) * 5 + ((out,) if p.degree == 0 else tuple(out))


def render(pool_params: PoolParams, rays: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0) -> dict:
    """{"rgb" [R, 3], "depth" [R], "opacity" [R]} of `rays` [R, 8] through the pool of `pool_params`, differentiable with respect
    to pool_params.rgbs, or to pool_params.coef and .sigma: forward upnerf_baked_sparse_render (at degree 1 | 2 on records packed
    from the parameters at level 0), backward upnerf_baked_sparse_render_bwd followed by upnerf_brick_face_sum -- every copy of a
    shared point receives the point's whole gradient.  No gradient for the rays.  With pool_params.env set: the march at background
    0 and the environment's composite after it, as in baked_tune.render."""
    if not isinstance(pool_params, PoolParams):
        raise ValueError("pool_params is a baked_sparse_tune.PoolParams (PoolParams.of(scene))")
    require_cuda("baked_sparse_tune.render", rays)
    step, background, stop = _render_args(rays, step, background, stop)
    rays = _rays16(rays)
    rgb, depth, opacity = _Render.apply(pool_params, rays, step, background if pool_params.env is None else 0.0, stop, *pool_params.tensors)
    if pool_params.env is not None:
        rgb = pool_params.env.composite(rays, rgb, opacity)
    return {"rgb": rgb, "depth": depth, "opacity": opacity}


class PoolTuner(BakedTuner):
    """Adam on the points of a sparse scene's pool against target pixels: baked_tune.BakedTuner's loop (upnerf_zero, forward, the
    MSE gradient, backward, upnerf_adam, upnerf_baked_project, at degree 1 | 2 upnerf_baked_sh_pack) with the sparse forward, the
    sparse backward and the face sum in it, every buffer flat over n_bricks * 729 points.  The table and the occupancy are the
    scene's and are frozen."""

    def _accept(self, scene) -> None:
        _sparse(scene, "PoolTuner")
        self.slots, self.bricks, self.resolution = scene.slots, scene.bricks, scene.resolution
        self._params = None  # the masters as a PoolParams, made on first use (the masters exist only after __init__)

    def _points(self, scene):
        P = _lib.BRICK_POINTS
        return (scene.n_bricks, P, P, P), scene.pool

    @property
    def params(self) -> PoolParams:
        """The masters as a PoolParams (the same memory, no gradient flags)."""
        if self._params is None:
            key = dict(rgbs=self.masters[0]) if self.degree == 0 else dict(coef=self.masters[0], sigma=self.masters[1])
            self._params = PoolParams(self.slots, self.bricks, self.occupancy, self.bounds, self.degree, **key)
        return self._params

    def _march(self, rays, step, background, stop):
        return _forward(self.points, self.params, rays, step, background, stop)

    def _gradient(self, rays, step, background, stop, g_rgb, g_opacity=None) -> None:
        """The marcher's gradient with the face sum; with the penalty on, the per-copy gradients of the marcher and of
        upnerf_baked_tv first and ONE face sum over both."""
        backward(self.points, self.params, rays, step, background, stop, g_rgb, g_opacity=g_opacity,
                 out=self.grads[0] if self.degree == 0 else self.grads, face_sum=not self.tv_on)
        if self.tv_on:
            from .baked_reg import tuner_tv
            self.last_tv = tuner_tv(self, layout=self.params)
            for t in self.grads:
                face_sum(t, self.params)

    @torch.no_grad()
    def scene(self) -> BakedScene:
        """The tuned sparse scene: the masters pruned again at the scene's level (upnerf_baked_pack / upnerf_baked_sh_pack over the
        pool), the same table, the bits from the pool (BakedScene._sparse)."""
        if self.degree == 0:
            rgbs = self.masters[0]
            sigma, rgb = rgbs[..., 3].contiguous(), rgbs[..., :3].contiguous()
            pool = torch.empty_like(rgbs)
            a = _lib.BakedPackArgs(n=sigma.numel(), level=self.level, sigma=ptr(sigma), rgb=ptr(rgb), rgbs=ptr(pool), kept=None)
            check(TIMER.run("baked_pack", lambda: lib.upnerf_baked_pack(C.byref(a), stream()), units=sigma.numel()), "upnerf_baked_pack")
        else:
            pool = pack_records(*self.masters, self.degree, self.level)
        return BakedScene._sparse(pool, self.slots, self.bricks, self.resolution, self.bounds, self.level, self.degree).with_environment(self.env)


def distill(system, scene: BakedScene, path_or_img_ids, iters: int, batch: int, baked_step: float, seed: int = 0, lr: float = 1e-2,
            img_id: Optional[int] = None, chunk: Optional[int] = None, tv: Tuple[float, float] = (0.0, 0.0), upsample_at=(),
            prune_at=(), prune_weight: Optional[float] = None):
    """baked_tune.distill for a sparse scene, tuned in place on its pool (PoolTuner): the same cameras, targets, batches and
    return value (the tuned SPARSE scene -- with the same bricks unless upsample_at refines it pool to pool -- and the loss curve);
    tv, upsample_at, prune_at and prune_weight as there (a pruned pool loses the bricks that are left empty)."""
    _sparse(scene, "distill")
    return _distill(PoolTuner, system, scene, path_or_img_ids, iters, batch, baked_step, seed, lr, img_id, chunk, tv, upsample_at,
                    prune_at, prune_weight)
