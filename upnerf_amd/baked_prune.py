"""Pruning a baked scene by what a set of rays sees (include/upnerf_hip.h: upnerf_baked_visibility, upnerf_brick_face_max,
upnerf_baked_prune; csrc/baked.hip, csrc/brick.hip).

    vis = scene.visibility(rays, step)                      # [Nz, Ny, Nx], or [n_bricks, 9, 9, 9] of a sparse scene
    small = scene.prune(rays, step)                         # what no ray sees is gone; those rays render to the same bits
    small = scene.prune(rays, step, min_weight=1e-3)        # Plenoxels' weight pruning: what no ray gives that much weight
    tuner = tuner.pruned(rays, step)                        # in a coarse-to-fine schedule, before tuner.upsampled()

`vis[p]` is the largest compositing weight w = T alpha that any of the rays gives a sample in a cell touching point p, and at
least 2^-126 (TINY_NORMAL) where a ray reaches such a cell with any light left: one more march through the forward's own walk,
reading the sigmas alone.  A maximum is exact and commutative, so the result has the same bits every run and however the rays
are cut into launches.  `prune` zeroes the points below `min_weight` in a copy and rebuilds the bits -- and, for a sparse scene,
the table: a brick none of whose points survives leaves the pool.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import BakedScene, _aligned, _aligned_copy, _common, _rays16, _render_args, a_scene, brick_face, brick_table, brick_words
from .ops import TIMER
from .static_scene import require_cuda

__all__ = ["visibility", "march_visibility", "prune", "prune_points", "face_max", "TINY_NORMAL"]

TINY_NORMAL = float(np.float32(2.0 ** -126))  # the smallest positive normal fp32: what a sample met with light left records at least


def _weight(min_weight) -> float:
    w = TINY_NORMAL if min_weight is None else float(min_weight)
    if w != w:
        raise ValueError("min_weight is not a number")
    return w


def face_max(t: torch.Tensor, scene: BakedScene) -> torch.Tensor:
    """upnerf_brick_face_max in place on the pool-shaped fp32 tensor `t` [n_bricks, 9, 9, 9, ...] of the sparse `scene`: every copy
    of a grid point that bricks share becomes the maximum over its copies.  Returns `t`."""
    if not a_scene(scene, "face_max").sparse:
        raise ValueError("face_max is for a sparse scene's pool-shaped tensors")
    return brick_face("max", t, scene.layout, "baked_prune.face_max")


def march_visibility(scene: BakedScene, rays: torch.Tensor, step: float, stop: float, vis: torch.Tensor) -> None:
    """One launch of upnerf_baked_visibility on checked arguments (_render_args, _rays16), maxed into `vis` (the per-copy values of
    a sparse scene: no face max)."""
    layout = scene.layout
    points, slots = layout.pointers(scene.points)
    common = _common(layout.occupancy, layout.bounds, rays, step, 0.0, stop)
    del common["background"]
    a = _lib.BakedVisibilityArgs(E=layout.point_bytes, sigma_offset=layout.sigma_at, points=points, slots=slots, vis=ptr(vis), **common)
    check(TIMER.run("baked_visibility", lambda: lib.upnerf_baked_visibility(C.byref(a), stream()), units=rays.shape[0]), "upnerf_baked_visibility")


@torch.no_grad()
def visibility(scene: BakedScene, rays: torch.Tensor, step: float, stop: float = 0.0, chunk: int = 16384) -> torch.Tensor:
    """The fp32 device tensor [Nz, Ny, Nx] (dense) or [n_bricks, 9, 9, 9] (sparse; after upnerf_brick_face_max, so the copies of
    a shared point are equal) of `rays` [R, 8] marched at `step` and `stop` as render marches them, `chunk` rays a launch.  The
    values do not depend on `chunk`."""
    a_scene(scene, "visibility")
    require_cuda("baked_prune.visibility", rays)
    step, _, stop = _render_args(rays, step, 0.0, stop)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    rays = _rays16(rays)
    vis = torch.zeros(scene.layout.shape, device=rays.device, dtype=torch.float32)
    if scene.sparse and scene.n_bricks == 0:
        return vis
    for r0 in range(0, rays.shape[0], chunk):
        march_visibility(scene, rays[r0:r0 + chunk], step, stop, vis)  # (a row is 32 bytes: every chunk stays 16-byte aligned)
    return face_max(vis, scene) if scene.sparse else vis


def prune_points(points: torch.Tensor, vis: torch.Tensor, E: int, min_weight: float, kept: Optional[torch.Tensor] = None) -> torch.Tensor:
    """upnerf_baked_prune in place on `points` (a contiguous device tensor of vis.numel() points of E bytes, 16-byte aligned): a
    point with NOT (vis >= min_weight) becomes a zero record.  kept: a uint8 tensor [vis.numel()] for the 1 / 0.  Returns `points`."""
    require_cuda("baked_prune.prune_points", points, vis)
    n = vis.numel()
    if vis.dtype != torch.float32 or not vis.is_contiguous() or not points.is_contiguous() or points.numel() * points.element_size() != n * E:
        raise ValueError(f"points are {n} contiguous points of {E} bytes beside a contiguous fp32 vis")
    if kept is not None and (kept.dtype != torch.uint8 or kept.numel() != n or not kept.is_contiguous() or kept.device != vis.device):
        raise ValueError(f"kept is a contiguous uint8 tensor of {n} on the points' device")
    a = _lib.BakedPruneArgs(n=n, min_weight=_weight(min_weight), E=E, vis=ptr(vis), points=ptr(points), kept=ptr(kept) if kept is not None else None)
    check(TIMER.run("baked_prune", lambda: lib.upnerf_baked_prune(C.byref(a), stream()), units=n), "upnerf_baked_prune")
    return points


@torch.no_grad()
def prune(scene: BakedScene, rays: torch.Tensor, step: float, min_weight: Optional[float] = None, stop: float = 0.0,
          chunk: int = 16384) -> BakedScene:
    """A new scene without the points whose visibility from `rays` is below `min_weight` (None: 2^-126, only what no ray sees);
    `scene` is not modified.  Dense: a copy of the grid is pruned and the bits rebuilt.  Sparse: a copy of the pool is pruned, the
    words rebuilt from it (upnerf_brick_occ) and the table from the words (upnerf_brick_table; one host read, the count), the
    surviving bricks selected through the old slots -- nothing the size of the grid is allocated.  env, level, bounds and
    sh_degree carry over.  At the default weight `rays` render at `step` and `stop` to the bits they rendered to before."""
    a_scene(scene, "prune")
    w = _weight(min_weight)
    degree, E = scene.sh_degree, scene.layout.point_bytes
    vis = visibility(scene, rays, step, stop, chunk)
    if not scene.sparse:
        grid = scene.grid.contiguous().view(torch.uint8)
        points = _aligned(grid.numel(), max(E, 16), grid.device)[:grid.numel()].view(grid.shape).copy_(grid)
        prune_points(points, vis, E, w)
        return BakedScene.from_points(points, scene.bounds, scene.level, degree).with_environment(scene.env)
    n, dev = scene.n_bricks, scene.device
    if n == 0:
        return scene.with_environment(scene.env)  # (nothing to drop: the same tensors)
    pool = scene.pool.contiguous().view(torch.uint8)
    points = _aligned(pool.numel(), E, dev)[:pool.numel()].view(pool.shape).copy_(pool)
    prune_points(points, vis, E, w)
    words = brick_words(points.view(-1), scene.slots, n, scene.resolution, E, scene.layout.sigma_at)
    slots, bricks, m = brick_table(words, scene.occupancy.dims)
    old = scene.slots.view(-1).index_select(0, bricks.long()).long()  # where each surviving brick lay in the old pool
    kept = _aligned_copy(points.index_select(0, old), E) if m else points[:0]
    return BakedScene._sparse(kept if degree else kept.view(torch.float32), slots, bricks, scene.resolution, scene.bounds, scene.level,
                              degree).with_environment(scene.env)
