"""Fine-tuning a SPARSE baked scene in place, on its brick pool: the marcher's backward pass through the pool
(`upnerf_baked_sparse_render_bwd`, csrc/baked.hip) and the sum over the copies of the points that bricks share
(`upnerf_brick_face_sum`, csrc/brick.hip); include/upnerf_hip.h states both; DESIGN.md 2.35.  The marcher's backward, the autograd
function, the tuner loop and distill are baked_tune.py's, written over a layout (baked.Layout); this module is their pool side:

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

from typing import Optional, Tuple

import torch

from .baked import DENSE_REFUSAL, BakedScene, Layout, a_scene, face_sum
from .baked_tune import BakedTuner, Params, _backward, _distill, _render

__all__ = ["PoolParams", "render", "backward", "face_sum", "PoolTuner", "distill", "DENSE_REFUSAL"]


def _sparse(scene, what: str) -> None:
    if not a_scene(scene, what).sparse:
        raise ValueError(DENSE_REFUSAL)
    if scene.n_bricks < 1:
        raise ValueError(f"{what}: the scene has no occupied brick, so nothing to tune")


class PoolParams(Params):
    """The fp32 parameters of a sparse scene over its pool, with what the marcher needs beside them: `rgbs`
    [n_bricks, 9, 9, 9, 4] at degree 0, else `coef` [n_bricks, 9, 9, 9, 3, nb] and `sigma` [n_bricks, 9, 9, 9]; the (frozen) table
    `slots` and `bricks`, the (frozen) occupancy, the bounds, the degree.  The tensors are leaves; `tensors` lists them."""

    noun = "pool"

    def __init__(self, slots, bricks, occupancy, bounds, degree: int, rgbs=None, coef=None, sigma=None, env=None):
        super().__init__(Layout(occupancy, bounds, degree, slots, bricks), rgbs, coef, sigma, env)

    @classmethod
    def of(cls, scene: BakedScene, requires_grad: bool = True) -> "PoolParams":
        _sparse(scene, "PoolParams.of")
        return cls._of(scene, requires_grad, scene.slots, scene.bricks, scene.occupancy, scene.bounds, scene.sh_degree)


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
    return _backward("baked_sparse_tune.backward", points, params.layout, rays, step, background, stop, g_rgb, g_depth, g_opacity, out,
                     face_sum)


def render(pool_params: PoolParams, rays: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0) -> dict:
    """{"rgb" [R, 3], "depth" [R], "opacity" [R]} of `rays` [R, 8] through the pool of `pool_params`, differentiable with respect
    to pool_params.rgbs, or to pool_params.coef and .sigma: forward upnerf_baked_sparse_render (at degree 1 | 2 on records packed
    from the parameters at level 0), backward upnerf_baked_sparse_render_bwd followed by upnerf_brick_face_sum -- every copy of a
    shared point receives the point's whole gradient.  No gradient for the rays.  With pool_params.env set: the march at background
    0 and the environment's composite after it, as in baked_tune.render."""
    if not isinstance(pool_params, PoolParams):
        raise ValueError("pool_params is a baked_sparse_tune.PoolParams (PoolParams.of(scene))")
    return _render("baked_sparse_tune.render", pool_params, rays, step, background, stop)


class PoolTuner(BakedTuner):
    """Adam on the points of a sparse scene's pool against target pixels: baked_tune.BakedTuner (upnerf_zero, forward, the MSE
    gradient, backward, upnerf_adam, upnerf_baked_project, at degree 1 | 2 upnerf_baked_sh_pack) on a pool's layout, which puts
    the sparse forward, the sparse backward and the face sum in it, every buffer flat over n_bricks * 729 points.  The table and
    the occupancy are the scene's and are frozen."""

    def _accept(self, scene) -> None:
        _sparse(scene, "PoolTuner")
        self.slots, self.bricks, self.resolution = scene.slots, scene.bricks, scene.resolution
        self._params = None  # the masters as a PoolParams, made on first use (the masters exist only after __init__)

    @property
    def params(self) -> PoolParams:
        """The masters as a PoolParams (the same memory, no gradient flags)."""
        if self._params is None:
            key = dict(rgbs=self.masters[0]) if self.degree == 0 else dict(coef=self.masters[0], sigma=self.masters[1])
            self._params = PoolParams(self.slots, self.bricks, self.occupancy, self.bounds, self.degree, **key)
        return self._params

    @torch.no_grad()
    def scene(self) -> BakedScene:
        """The tuned sparse scene: the masters pruned again at the scene's level (upnerf_baked_pack / upnerf_baked_sh_pack over the
        pool), the same table, the bits from the pool (BakedScene._sparse)."""
        pool = self._pruned_points()
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
